/* piccolo_hip.h — C ABI of the MI355X (gfx950) implementation of PICCOLO's sampling-loss hot path.
 *
 * The reference (82magnolia/piccolo) is pure Python/PyTorch and has no FFI layer; its boundary for this path is
 * the Python surface omniloc.py / utils.py.  This header is what a ctypes binding of that surface calls
 * (see INTEGRATION.md for the stub).  Each entry point cites the reference code it replaces
 * (file:line relative to the reference checkout).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host; all buffers are caller-owned, the device entry
 *    points never allocate, free or synchronise (graph-capture safe); `stream` is a hipStream_t passed as void*;
 *    the dataset text reader (pcl_cloud_txt_*) is host-only code and takes host pointers;
 *  - every function returns 0 on success, a hipError_t value (> 0) for a runtime failure, or one of the
 *    negative PCL_E* codes below for a bad argument;
 *  - fp32 throughout, like the reference (localize.py:159-170); poses are (t[3], yaw, pitch, roll) with
 *    p = R (x - t), R = RZ(yaw) RY(pitch) RX(roll)  (utils.py:425-453).
 */
#ifndef PICCOLO_HIP_H
#define PICCOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCL_ABI_VERSION 12 /* 12: room search over several panoramas — images x rooms in one chain (pcl_gd_rooms_images_workspace_bytes, pcl_gd_plan_rooms_images, pcl_gd_init_rooms_images, pcl_gd_run_rooms_images); 11: room search — several clouds in one refinement chain (pcl_gd_room, pcl_gd_rooms_workspace_bytes, pcl_gd_plan_rooms, pcl_gd_run_rooms); 10: per-image colour sets (pcl_cloud_sets_bytes / pcl_cloud_pack_sets, pcl_gd_hyper.color_sets, pcl_trim_loss_images_sets, pcl_hist_trim_*_sets); 9: pcl_gd_hyper.fuse, pcl_loss_depth_workspace_bytes takes the occluder stride, pcl_trim_order + the `order` argument of pcl_trim_loss[_images], the library reads no environment variable; 8: PCL_PANO_U8V / pcl_pano_pack_u8v; 7: depth mask on its own grid (pcl_gd_hyper.depth_h / depth_w, pcl_depth_default, pcl_sampling_loss_depth), refresh rule and pcl_gd_depth_refresh_counts removed, pcl_gd_step_from_grads; 6: pcl_select_poses, pcl_gd_set_pano_groups, pcl_gd_winner; 2: fp16-level texels, colour preprocessing, histograms, dataset text reader; 3: backward of the stand-alone ops; 4: pcl_hist_trim_workspace_bytes_n; 5: pcl_source_hash, pcl_timer_calibrate, pcl_trim_*, pcl_gd_plan */

#define PCL_EINVAL (-1)   /* bad size / null pointer / unsupported argument */
#define PCL_EWORKSPACE (-2) /* workspace too small */

/* largest cloud of the loss / refinement / ordering entry points: the six planes of the packed cloud are addressed through one
 * 32-bit buffer descriptor (6 x 4 B x n < 4 GiB); a larger n is answered with PCL_EINVAL before anything is enqueued */
#define PCL_MAX_POINTS ((int64_t)1 << 27)

/* number of floats per pose in result blocks: loss, count, dL/dt[3], dL/dyaw, dL/dpitch, dL/droll */
#define PCL_RESULT_STRIDE 8

int pcl_abi_version(void);
const char *pcl_error_string(int code);
/* Which sources the loss kernel of THIS binary was compiled from: the first 16 hex digits of sha256(csrc/pcl_loss.hip +
 * csrc/pcl_sample_device.h + csrc/pcl_gd_device.h + csrc/pcl_device.h), stamped in by piccolo_amd/build.py ("unstamped" for a build that did not pass -DPCL_SOURCE_HASH).
 * Measurement aid: counter-derived figures (VALU instructions per point-pose, profiles/roofs.json) carry the hash of the
 * library they were collected from, and bench.py reports them only for a library with the same hash. */
const char *pcl_source_hash(void);
/* The same over EVERY source of the library (all .hip and .h files of csrc, this header): what the per-kernel roofs of the pipeline kernels
 * (trim, bin / resolve, z pass: profiles/pipeline_roofs.json) are stamped with. */
const char *pcl_library_hash(void);

/* ---- data layout in HBM ------------------------------------------------------------------------------------
 * cloud : 6 planes (x, y, z, -r, -g, -b) of pcl_cloud_stride(n) floats each (colours negated: the loss needs c - rgb) — SoA so that a wavefront's 64 lanes
 *         read 256 contiguous bytes per plane.  Built once per point cloud from the reference's row-major
 *         (N,3) xyz and rgb tensors (localize.py:159-164).  `order` (nullable, int64[n]) gathers
 *         point order[i] into slot i: passing a space-filling-curve order makes consecutive lanes hit
 *         neighbouring texels (the loss is a sum over points, so the order does not change the result beyond
 *         fp32 summation rounding).
 * pano  : the query image (H,W,3) float (localize.py:167-170) repacked as (H+2, W+2) texels with a one-texel zero
 *         border, so grid_sample's zero padding (utils.py:98) needs no bounds test.  Three texel formats:
 *           PCL_PANO_F32 : RGBA float4, 16 B/texel — any float image;
 *           PCL_PANO_U8  : RGBA8, 4 B/texel — for images whose every value is exactly k/255 in fp32, which is what
 *                          the reference always feeds (cv2.imread -> uint8 -> .float() / 255., localize.py:167-170,
 *                          211-213; color_mod also re-quantises to uint8, color_utils.py:48-50).  A 2x2 bilinear
 *                          footprint is then two 8-byte loads and the whole panorama is 4x smaller, so the gathers
 *                          stay in L2.  The kernel interpolates the integer levels and scales by 1/255 once.
 *           PCL_PANO_F16 : RGBA half4, 8 B/texel — the same k/255 images with the levels 0..255 held as fp16 (exact).
 *                          A footprint is two 16-byte loads; the tap differences are exact fp16 and the lerps read
 *                          fp16 operands directly (v_fma_mix_f32), so no tap is converted: same results as PCL_PANO_U8
 *                          bit for bit, loss kernel 4-5 % faster, twice the texture bytes (still L2/MALL resident).
 *         pcl_pano_pack_u8 / _f16 set *not_exact (device int, caller zeroes it) if some value is NOT exactly k/255:
 *         the caller must then fall back to PCL_PANO_F32.
 */
#define PCL_PANO_F32 0
#define PCL_PANO_U8 1
#define PCL_PANO_F16 2
/* PCL_PANO_U8P: RGBA8 with the ROWS INTERLEAVED IN PAIRS — element (x, k) = 8 bytes = texel (x, 2k), texel (x, 2k + 1) of the bordered
 * image, element rows of W + 2 elements.  A 2 x 2 footprint that starts on an even row is ONE 16-byte access, on an odd row two:
 * 1.5 texture accesses per sample on average instead of 2, with the memory of PCL_PANO_U8.  Only the forward-only trim launch takes
 * it (pcl_trim_loss / pcl_trim_loss_images: bound by the texture unit's line rate); pcl_pano_pack_u8p packs it. */
#define PCL_PANO_U8P 3
/* PCL_PANO_U8V: RGBA8 in VERTICAL PAIRS — element (x, y) = 8 bytes = texel (x, y), texel (x, y + 1) of the bordered image, H + 2 element
 * rows of W + 2 elements.  Every 2 x 2 footprint is ONE 16-byte access, for twice the texture bytes of PCL_PANO_U8.  Only the trim
 * launch takes it (dense clouds, where that launch is bound by texture accesses and VALU issue alike); pcl_pano_pack_u8v packs it. */
#define PCL_PANO_U8V 4
int64_t pcl_cloud_stride(int64_t n);
size_t pcl_cloud_bytes(int64_t n);
int pcl_cloud_pack(const float *xyz, const float *rgb, const int64_t *order, int64_t n, float *cloud, void *stream);
/* Per-image colour sets (ABI 10): ONE point set with nsets colourings — e.g. the reference's color_mod, which gives every query image its
 * own equalised cloud colours (localize.py:173-179) — as planes x, y, z, then nsets x (-r, -g, -b), each pcl_cloud_stride(n) floats.
 * nsets = 1 is pcl_cloud_pack's 6-plane cloud, byte for byte.  rgb_host = HOST array of nsets device addresses of (n, 3) colours; the
 * same Morton `order` gathers every plane.  Colour set k is a scalar plane offset on the cloud's one 32-bit buffer descriptor, so the whole
 * cloud must stay below 2^31 bytes: (3 + 3 nsets) x 4 x pcl_cloud_stride(n) < 2^31 — 177 sets at 1M points (stride 1,000,192), 16 at 10M.
 * pcl_cloud_sets_bytes answers 0 beyond that (or for n > PCL_MAX_POINTS, nsets < 1) and every entry point that takes a set count answers
 * PCL_EINVAL: the caller splits its images into groups. */
size_t pcl_cloud_sets_bytes(int64_t n, int nsets);
int pcl_cloud_pack_sets(const float *xyz, const float *const *rgb_host, int nsets, const int64_t *order, int64_t n, float *cloud, void *stream);
/* Per-point weights (build-defined: the reference has none and treats every point alike).  A cloud may carry ONE weight per point, w_i >= 0
 * and finite, shared by all poses of a call, in a plane of its own: pcl_cloud_stride(n) floats in the PACKED point order,
 * plane[s] = w[order ? order[s] : s] with `order` the one given to pcl_cloud_pack, padding slots 0.  pcl_cloud_weights_bytes(n) is its size
 * (0 for n <= 0 or n > PCL_MAX_POINTS).  pcl_cloud_pack_weights sets *bad (device int, caller zeroes it) if some weight is negative, NaN or
 * infinite: the plane must then not be used.  The plane's address is the caller's: re-packing into the same buffer changes the weights
 * that a captured graph of pcl_gd_run_weighted reads.  With weights
 *   loss_b      = sum_i w_i m_bi ||c_bi - rgb_i|| / sum_i w_i m_bi             (0/0 -> NaN, as for an empty mask)
 *   grad loss_b = sum_i w_i m_bi grad ||c_bi - rgb_i|| / sum_i w_i m_bi        (m is piecewise constant, as in the reference's autograd)
 *   result[1] ("count") = sum_i w_i m_bi                                       (a float; the point count when w = 1)
 * Unit weights give the unweighted results bit for bit, 0/1 weights those of the same byte mask `visible`.
 * Deliberately left out: weights in the initialisation stage (pcl_trim_*, pcl_hist_trim_*), in the rooms and rooms x images chains and
 * under the depth mask, caller-brought weights in the images / colour-set chains (one plane per query image exists for the robust chain:
 * pcl_gd_run_weight_sets below), and a semantic source of weights — the caller brings them, or makes them
 * from the residuals of a pose with pcl_point_residuals / pcl_robust_weights below, from a score map (pcl_score_weights), or from the
 * sampling density (pcl_voxel_grid / pcl_density_weights). */
size_t pcl_cloud_weights_bytes(int64_t n);
int pcl_cloud_pack_weights(const float *w, const int64_t *order, int64_t n, float *plane, int32_t *bad, void *stream);
/* Per-point residuals (additive to ABI 12; build-defined, one cloud with one colour set, no depth mask — the scope of the weights they feed):
 * what the loss kernel sums, before it is summed.  For pose b = (trans + b * pose_stride, rot + b * pose_stride: yaw, pitch, roll)
 *   residual[b][i] = ||c_bi - rgb_i||   where pcl_sampling_loss's mask keeps point i (the n2 * rsq(n2 + 1e-37) the loss kernel adds),
 *                  = -1.0f exactly      where the sampled colour is exactly (0, 0, 0) and the point is masked;
 * a pose that holds a NaN or an infinity sees nothing: its whole row is NaN (neither kept nor masked).  At a finite pose (row >= 0).sum() is pcl_sampling_loss's count, bit for bit, and the sum
 * of the kept entries its loss numerator up to the summation order.  pose_stride = 3 reads plain [B][3] arrays; pose_stride = 16 with
 * trans = winners, rot = winners + 13 reads the rows pcl_gd_winner wrote, on the device.  order == NULL: packed slot order,
 * residual[b][s]; order = the order given to pcl_cloud_pack: the caller's point order, residual[b][order[s]].  Rows are n floats apart.
 * One launch (256-thread blocks, two points per lane, chunks x poses), forward only, no workspace, no atomics; capturable.
 * PCL_EINVAL, before any HIP call: a null cloud / pano / trans / rot / residual, n outside 1..PCL_MAX_POINTS, B <= 0 or more blocks than a
 * grid holds, H or W <= 0, a packed panorama of 2 GiB, the trim-only texel formats PCL_PANO_U8P / PCL_PANO_U8V, pose_stride < 3. */
int pcl_point_residuals(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans, const float *rot,
                        int pose_stride, int B, const int64_t *order, float *residual, void *stream);
/* The same for nimages poses, each against ITS OWN panorama (additive to ABI 12): row i is the residual row of pose i (trans + i * pose_stride, rot
 * + i * pose_stride) against panos_host[i] (HOST array of nimages device addresses of packed panoramas of one H, W and texel format) and, when
 * color_sets == nimages, colour set i of a cloud of pcl_cloud_pack_sets (color_sets 0 / 1: the cloud's one set).  Row i equals what
 * pcl_point_residuals returns for that pose, panorama and colour set alone, bit for bit: the same kernel body.  The addresses travel as kernel
 * arguments (one launch per 64 images): nothing is copied, nothing waits for the host, capturable.  pose_stride = 16 with trans = winners,
 * rot = winners + 13 reads pcl_gd_winner's [nimages][16] rows on the device.
 * PCL_EINVAL, before any HIP call: what pcl_point_residuals refuses (B = nimages), a null panos_host or a null entry, color_sets < 0 or
 * > 1 and not nimages, a cloud of color_sets sets past the addressing limit (pcl_cloud_sets_bytes answers 0). */
int pcl_point_residuals_images(const float *cloud, int64_t n, int color_sets, const uint64_t *panos_host, int nimages, int pano_format, int H, int W,
                               const float *trans, const float *rot, int pose_stride, const int64_t *order, float *residual, void *stream);
/* Robust weights from ONE residual row in packed order (residual_packed[n]; M = the number of entries that are not -1):
 *   s = the lower median of those entries, the element of 0-based rank (M - 1) / 2 in ascending order — exact, by an MSB radix select over
 *       the bit patterns with integer atomics only, so it does not depend on scheduling (every NaN ranks as one value behind +inf);
 *   c = k * s (one fp32 multiply);
 *   plane[slot] = 1 where the entry is -1 (masked at this pose: no evidence either way),
 *                 PCL_ROBUST_TRUNC: l <= c ? 1 : 0,    PCL_ROBUST_HUBER: l <= c ? 1 : c / l (IEEE division; 0 when c is NaN),
 *                 0 for a NaN or infinite entry under both kinds;  M == 0: every weight 1 and s = 0.
 * `plane` is the packed plane pcl_gd_run_weighted reads: pcl_cloud_stride(n) floats, padding 0; it may be written in place of an older
 * one.  scale_out (nullable, device float[2]) receives s and M (as a float: exact up to 2^24).  Six launches, capturable.
 * PCL_EINVAL, before any HIP call: a null residual / plane / workspace, n outside 1..PCL_MAX_POINTS, an unknown kind, k <= 0 or not
 * finite, workspace_bytes below pcl_robust_weights_workspace_bytes(n) (0 for n out of range). */
#define PCL_ROBUST_TRUNC 0
#define PCL_ROBUST_HUBER 1
size_t pcl_robust_weights_workspace_bytes(int64_t n);
int pcl_robust_weights(const float *residual_packed, int64_t n, int kind, float k, float *plane, float *scale_out, void *workspace,
                       size_t workspace_bytes, void *stream);
/* pcl_robust_weights for nrows rows in the SAME six launches (additive to ABI 12; the row is the grid's second dimension, so the launch count
 * does not grow with the rows): residual_packed [nrows][n] (rows n floats apart), planes [nrows][pcl_cloud_stride(n)], scale_out (nullable)
 * [nrows][2].  Every row has its own histograms in the workspace, pcl_robust_weights_rows_workspace_bytes(n, nrows) (0 for n out of range or
 * nrows outside 1..65535).  Plane i and scale_out[i] equal pcl_robust_weights of row i alone, bit for bit (integer atomics only; a row
 * with M = 0 or NaN entries behaves as there).  PCL_EINVAL, before any HIP call: as pcl_robust_weights, nrows outside 1..65535. */
size_t pcl_robust_weights_rows_workspace_bytes(int64_t n, int nrows);
int pcl_robust_weights_rows(const float *residual_packed, int64_t n, int nrows, int kind, float k, float *planes, float *scale_out, void *workspace,
                            size_t workspace_bytes, void *stream);
/* Score maps (additive to ABI 12; BUILD-DEFINED: the reference reduces the histogram stage's evidence to one number per pose).  Inputs: a
 * packed cloud of pcl_cloud_pack (one colour set, no weights), K poses trans[K][3] / rot[K][3], the panorama size H x W, a split nsh x nsw
 * (bh = H / nsh, bw = W / nsw, nblk = (nsh - 2) nsw) and pcl_hist_trim_scores' inter[K][nblk], nproj[K][nblk], nimg[nblk] for exactly these
 * poses and this split.  valid(k, j) = nproj[k][j] > 0 && nimg[j] > 0 (the slot carry-over of pcl_hist_trim_reduce plays no part).
 *   score2d[j], count2d[j]   the fp32 sum of inter[k][j] over the valid k in ascending order / their number (one IEEE division; exactly -1
 *                            where the count is 0);
 *   score3d[p], count3d[p]   the same over the poses k for which point p's centre pixel — the render's: R (x - t), truncate, clamp, no
 *                            wrap — lies in a scored block j (h = row / bh in 1 .. nsh - 2, w = col / bw < nsw) with valid(k, j).  A pose
 *                            that is not finite casts no vote.  No occlusion test: a hidden point votes with the patch in front of it.
 * order null: score3d / count3d in packed order; otherwise order[slot] is the caller's index of the packed point (pcl_cloud_pack's order)
 * and the outputs are in the caller's order.  Either pair of outputs may be null, not both.  Two launches, no atomics: the result does not
 * depend on scheduling; nothing is allocated, nothing waits for the host (capturable).
 * PCL_EINVAL, before any HIP call: a null input or workspace, both output pairs null or half a pair, n outside 1..PCL_MAX_POINTS, K outside
 * 1..65535, nsh < 3, nsw < 1, H or W outside 1..65535, a block of zero pixels, workspace_bytes below pcl_score_maps_workspace_bytes(n, K,
 * nsh, nsw) (0 for a shape no call accepts). */
size_t pcl_score_maps_workspace_bytes(int64_t n, int K, int nsh, int nsw);
int pcl_score_maps(const float *cloud, int64_t n, const float *trans, const float *rot, int K, int H, int W, int nsh, int nsw, const float *inter,
                   const int32_t *nproj, const int32_t *nimg, const int64_t *order, float *score3d, int32_t *count3d, float *score2d,
                   int32_t *count2d, void *workspace, size_t workspace_bytes, void *stream);
/* A weight plane from a 3D score map given in any one point order (score_packed[n], count_packed[n]; scores >= 0 wherever the count is at
 * least min_count).  lo / hi = the smallest / largest score over the points with count >= min_count (`voted` of them), by integer atomic
 * min / max on the bit patterns: the result does not depend on scheduling.
 *   plane[i] = clamp(fma(1 - floor, (s - lo) / (hi - lo), floor), 0, 1) for such a point, every operation rounded once, in this order;
 *              1 for a point with fewer votes (no evidence), and for every point when voted == 0 or hi == lo.
 * `plane` is the packed plane pcl_gd_run_weighted reads: pcl_cloud_stride(n) floats, padding 0.  range_out (nullable, device float[3])
 * receives lo, hi (0, 0 when nothing voted) and voted (as a float).  Three launches, capturable.
 * PCL_EINVAL, before any HIP call: a null score / count / plane / workspace, n outside 1..PCL_MAX_POINTS, min_count < 1, floor outside
 * [0, 1), workspace_bytes below pcl_score_weights_workspace_bytes(n) (0 for n out of range). */
size_t pcl_score_weights_workspace_bytes(int64_t n);
int pcl_score_weights(const float *score_packed, const int32_t *count_packed, int64_t n, int min_count, float floor, float *plane, float *range_out,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Pose information matrix and covariance (additive to ABI 12; BUILD-DEFINED: the reference returns a pose and a loss and says nothing about
 * how well the panorama constrains the pose).  One cloud with one colour set, no depth mask, as the residuals above.  For pose b =
 * (trans + b * pose_stride, rot + b * pose_stride: yaw, pitch, roll), theta = (t0, t1, t2, yaw, pitch, roll), and per point i the loss
 * kernel's mask bit m_i (sampled colour not exactly black), its weight w_i (1 when weights == NULL; otherwise the packed plane of
 * pcl_cloud_pack_weights / pcl_robust_weights), its residual l_i = ||c_i - rgb_i|| and j_i = d l_i / d theta (6), the per-point term
 * [grad_t, grad_ypr] that pcl_sampling_loss sums: j = C a, a = [g; tau], g = d l / d p in the camera frame, tau = p x g, and
 *   grad_t = -R^T g;  yaw = tau_z;  pitch = -sin(yaw) tau_x + cos(yaw) tau_y;  roll = cy cp tau_x + sy cp tau_y - sp tau_z:
 *   M = sum w m     S1 = sum w m l     S2 = sum w m l^2     H = sum w m j j^T (6 x 6, symmetric)     b = sum w m l j (6)
 *   sigma^2 = S2 / M          cov = sigma^2 H^-1 (6 x 6, symmetric bit for bit; theta's units: metres for t, radians for the angles)
 * w enters linearly (one factor per term, never squared).  info[b] is 48 floats: H row-major (36), b (6), M, S1, S2, sigma^2, status, 0.
 * cov (nullable) is [B][36].  status: 0 fine; 1: M = 0, or a pose or a sum that is not finite — H and b are reported as summed, cov is
 * all NaN; 2: H is not positive definite in double (a Cholesky pivot <= 6 * 2^-52 * the largest diagonal entry) — cov is all NaN.
 * Nothing aborts.  Two launches: 256-thread blocks over chunks x poses accumulate the 30 sums in fp32 per lane and reduce them in a
 * fixed order into one partial row per (chunk, pose) in the workspace, then one block per pose adds the rows, applies C, factorises and
 * inverts in double and rounds every output once.  No atomics, no allocation, no synchronisation: capturable; the same inputs give the
 * same bits.  pose_stride as for pcl_point_residuals (16 with trans = winners, rot = winners + 13 reads pcl_gd_winner's rows in place).
 * Weights scaled by a power of two scale H, b, M, S1, S2 by it and cov by its inverse and change no other bit.
 * pcl_pose_information_workspace_bytes(n, B): 0 for n outside 1..PCL_MAX_POINTS, B <= 0 or more blocks than a grid holds.
 * PCL_EINVAL, before any HIP call: what pcl_point_residuals refuses (null cloud / pano / trans / rot, n, B, H, W, a 2 GiB panorama, the
 * trim-only texel formats PCL_PANO_U8P / PCL_PANO_U8V, pose_stride < 3), a null info or workspace, workspace_bytes below the query's.
 * Deliberately left out: colour sets, the images / depth chains (the rooms chains: pcl_pose_information_rooms), a Gauss-Newton step on H
 * and b, and any claim that cov is calibrated on real data (sigma^2 is the mean squared colour residual of the kept points, nothing more). */
size_t pcl_pose_information_workspace_bytes(int64_t n, int B);
int pcl_pose_information(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                         const float *rot, int pose_stride, int B, float *info, float *cov, void *workspace, size_t workspace_bytes, void *stream);
/* Levenberg-Marquardt pose polish on H and b (additive to ABI 12; BUILD-DEFINED: the reference refines with Adam and has nothing like it).
 * What is minimised is the MEAN SQUARED residual sigma^2(theta) = sum w m l^2 / sum w m over theta = (t0, t1, t2, yaw, pitch, roll), with m, w,
 * l, H and b those of pcl_pose_information above.  It is NOT the sampling loss sum w m l / sum w m that the pcl_gd_* chains minimise: the two
 * share their per-point terms, mask and weights and are different objectives.  Units: metres for t, radians for the angles; step_cap and
 * tol bound both alike.  The whole chain runs on the device: one call enqueues an init launch and, for every evaluation k = 0 .. iters, a
 * per-point pass launch at the trial pose (pcl_pose_information's pass, same arithmetic and partial rows, with the poses read from the
 * state; the blocks of a frozen pose return before their point loop) and a step launch (one block per pose):
 *   F = (float)(S2 / M) from the rows added in double in pcl_pose_information's order.  The trial is ACCEPTED iff the sums are finite,
 *   M > 0 and F < F_acc compared in fp32 (F_acc = +inf at the start; evaluation 0 is accepted iff the sums are finite and M > 0, else the pose
 *   freezes with status 1 and the caller's pose is returned).  On acceptance theta_acc, F_acc, H, b and the stats become the trial's and,
 *   except at k = 0, lambda = fmaxf(lambda * lam_down, lam_min); on rejection lambda = fminf(lambda * lam_up, lam_max).
 *   Step (none after evaluation `iters`): (H + lambda diag H) delta = -b in double on the ACCEPTED H and b, by pcl_pose_information's Cholesky
 *   with its power-of-two scaling (a failed pivot freezes the pose with status 2); if max |delta_i| > step_cap the whole delta is scaled by
 *   step_cap / max |delta_i|; theta_try = (float)((double)theta_acc + delta).  The pose freezes converged, status 3, when max |delta_i| <= tol
 *   or theta_try equals theta_acc in all six floats.  A frozen pose takes no further part.
 * out[b] is 16 floats: theta_acc (6), F at the start, F_acc, the final lambda, accepted, rejected, evaluations, status, 0, 0, 0.
 * status: 0 all evaluations ran; 1 the first evaluation had M = 0 or something not finite; 2 the damped matrix was not positive
 * definite; 3 converged.  info[b] (48 floats) and cov[b] (nullable, 36) are pcl_pose_information's record and covariance at theta_acc, formed
 * from the accepted sums by the same code: the same bits as that call at that pose.  trace (nullable) is [iters + 1][B][16]: per
 * evaluation theta_try (6), F, accepted 0/1, lambda after the decision, M, 0 x 6; rows a frozen pose never reached are 0.
 * pcl_gn_hyper is read on the host when the call is enqueued (a captured graph keeps its values).  Defaults of the package: lam0 1e-3,
 * lam_up 10, lam_down 0.1, lam_min 1e-9, lam_max 1e9, step_cap 0.1, tol 0 (never converged by size).
 * state: pcl_gn_state_bytes(B) bytes the caller owns (0 for B <= 0), written by the init launch; workspace: pcl_gn_workspace_bytes(n, B)
 * (0 for a bad n or B).  No atomics, no allocation, no synchronisation: capturable; the same inputs give the same bits, and pose b of a
 * batch has the bits of its own call.  Weights scaled by a power of two change no pose, no lambda, no flag and no F.
 * PCL_EINVAL, before any HIP call: everything pcl_pose_information refuses; iters < 0 or > 1000; a null hyper_host, state, out or info; a
 * hyper-parameter that is not finite; lam0 <= 0, lam_up <= 1, lam_down <= 0 or > 1, lam_min > lam_max, step_cap <= 0, tol < 0.
 * Deliberately left out: an IRLS form that minimises the sampling loss itself, re-weighting inside the chain, the box clamp of the
 * reference's refinement, colour sets, the images / depth chains (the rooms chains: pcl_gn_refine_rooms), and any claim about real data. */
typedef struct pcl_gn_hyper {
    float lam0, lam_up, lam_down, lam_min, lam_max, step_cap, tol;
} pcl_gn_hyper;
size_t pcl_gn_state_bytes(int B);
size_t pcl_gn_workspace_bytes(int64_t n, int B);
int pcl_gn_refine(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                  const float *rot, int pose_stride, int B, const pcl_gn_hyper *hyper_host, int iters, void *state, float *out, float *info,
                  float *cov, float *trace, void *workspace, size_t workspace_bytes, void *stream);
/* pcl_pose_information and pcl_gn_refine for the nimages winners of a chain over several query images of one cloud, in ONE set of launches
 * (additive to ABI 12; BUILD-DEFINED): pose i = (trans + i * pose_stride, rot + i * pose_stride) is evaluated against panos_host[i] (HOST
 * array of nimages device addresses of packed panoramas of one H, W and texel format; they travel as kernel arguments, 64 per pass launch:
 * nothing is copied, nothing waits for the host, capturable), against colour set i of a cloud of pcl_cloud_pack_sets when color_sets ==
 * nimages (color_sets 0 / 1: the cloud's one set, pcl_point_residuals_images' rule), and under
 *   weights == NULL, weight_sets == 0         no weights;
 *   weight_sets == 1                          the one packed plane `weights` for every image;
 *   weight_sets == nimages                    plane i at weights + i * pcl_cloud_stride(n) (pcl_robust_weights_rows' layout; the planes of
 *                                             pcl_gd_run_weight_sets).
 * Record i (info, cov; for pcl_gn_refine_images also out, the state and the trace rows [iters + 1][nimages][16]) equals what
 * pcl_pose_information / pcl_gn_refine returns for that pose, panorama, colour set and plane alone, bit for bit: the same per-point pass
 * over chunks that depend on n only, the same partial rows, and the per-pose finish / init / step kernels themselves.  Poses never
 * interact; the blocks of a frozen pose return before their point loop, per pose.  More than 64 images run in groups of 64 inside the
 * call (one pass launch per group and evaluation; colour set and plane are counted from the call's first image).  Sizes:
 * pcl_pose_information_workspace_bytes(n, nimages), pcl_gn_state_bytes(nimages), pcl_gn_workspace_bytes(n, nimages).  No atomics, no
 * allocation, no synchronisation.
 * PCL_EINVAL, before any launch: what pcl_pose_information / pcl_gn_refine refuse (B = nimages); a null panos_host or a zero entry;
 * weights == NULL with weight_sets != 0, weights with a weight_sets that is neither 1 nor nimages; color_sets < 0, or > 1 and not nimages;
 * weight planes or colour sets of 2^31 bytes or more together (one buffer resource each).
 * Deliberately left out: of the rooms and depth chains the depth chains (the rooms chains have pcl_pose_information_rooms /
 * pcl_gn_refine_rooms, declared next to pcl_gd_run_rooms_images), a forward-only loss launch for a colour set or a per-image plane (the
 * weighted sampling loss at a returned pose is S1 / M of its info record), and any claim that cov is calibrated on real data. */
int pcl_pose_information_images(const float *cloud, const float *weights, int weight_sets, int64_t n, int color_sets, const uint64_t *panos_host,
                                int nimages, int pano_format, int H, int W, const float *trans, const float *rot, int pose_stride, float *info,
                                float *cov, void *workspace, size_t workspace_bytes, void *stream);
int pcl_gn_refine_images(const float *cloud, const float *weights, int weight_sets, int64_t n, int color_sets, const uint64_t *panos_host, int nimages,
                         int pano_format, int H, int W, const float *trans, const float *rot, int pose_stride, const pcl_gn_hyper *hyper_host,
                         int iters, void *state, float *out, float *info, float *cov, float *trace, void *workspace, size_t workspace_bytes,
                         void *stream);
/* The Huber-L1 forms of the four calls above (additive to ABI 12; BUILD-DEFINED): a polish that minimises, for
 * delta -> 0, the sampling loss itself.  Per kept point with residual l >= 0 and delta > 0
 *   phi(l) = min(1 / l, 1 / delta)                              the IRLS weight (l = 0: 1 / delta)
 *   rho(l) = l >= delta ? l - delta / 2 : l^2 / (2 delta)       Huber's function divided by delta: C^1, rho' = phi l, -> l as delta -> 0
 *   F_rho = sum w m rho / sum w m     H_rho = sum w m phi j j^T     b_rho = sum w m phi l j
 * The parameters are the twin's without `cov`, plus `float delta` before the stream.  The 48-float record holds H_rho (0..35), b_rho
 * (36..41), M (42) and S1 (43) — both PLAIN, no phi: S1 / M is the weighted sampling loss at the pose —, sum w m rho (44), F_rho (45) and
 * the status (46).  In pcl_gn_refine_l1 / pcl_gn_refine_images_l1 the chain decides on F_rho and solves (H_rho + lambda diag H_rho) d =
 * -b_rho; the `out` and trace columns that hold sigma^2 in the twin hold F_rho.  For delta >= max l the record's H, b are the twin's
 * divided by delta and slot 44 is S2 / (2 delta).  No covariance is offered: F_rho H_rho^-1 is not the twin's.  Only the per-point pass
 * differs from the twin (an instance of the same kernel text); the init, step and finish kernels, the state, the sizes
 * (pcl_pose_information_workspace_bytes, pcl_gn_workspace_bytes, pcl_gn_state_bytes), the launch counts, the gate on frozen poses and the
 * bit-for-bit independence of poses and images are the twin's.  No atomics, no allocation, no synchronisation: capturable.
 * PCL_EINVAL, before any launch: what the twin refuses; a delta that is not finite or lies outside [2^-20, 4] as a float (residuals
 * never exceed sqrt(3)).  Deliberately left out: a rooms form, the depth mask, any claim about real data. */
int pcl_pose_information_l1(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                            const float *rot, int pose_stride, int B, float *info, void *workspace, size_t workspace_bytes, float delta,
                            void *stream);
int pcl_pose_information_images_l1(const float *cloud, const float *weights, int weight_sets, int64_t n, int color_sets, const uint64_t *panos_host,
                                   int nimages, int pano_format, int H, int W, const float *trans, const float *rot, int pose_stride, float *info,
                                   void *workspace, size_t workspace_bytes, float delta, void *stream);
int pcl_gn_refine_l1(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                     const float *rot, int pose_stride, int B, const pcl_gn_hyper *hyper_host, int iters, void *state, float *out, float *info,
                     float *trace, void *workspace, size_t workspace_bytes, float delta, void *stream);
int pcl_gn_refine_images_l1(const float *cloud, const float *weights, int weight_sets, int64_t n, int color_sets, const uint64_t *panos_host,
                            int nimages, int pano_format, int H, int W, const float *trans, const float *rot, int pose_stride,
                            const pcl_gn_hyper *hyper_host, int iters, void *state, float *out, float *info, float *trace, void *workspace,
                            size_t workspace_bytes, float delta, void *stream);
/* The Morton order in one call, entirely on the device: bounding box, 63-bit keys, stable radix sort of (key, index);
 * order[i] = index of the point for packed slot i.  workspace: pcl_cloud_order_workspace_bytes(n). */
size_t pcl_cloud_order_workspace_bytes(int64_t n);
int pcl_cloud_order(const float *xyz, int64_t n, int64_t *order, void *workspace, size_t workspace_bytes, void *stream);
/* 63-bit Morton keys of xyz quantised to 21 bits per axis inside [lo, hi] (host arrays of 3); sort them to get `order`. */
int pcl_morton_keys(const float *xyz, int64_t n, const float *lo_host, const float *hi_host, int64_t *keys, void *stream);
/* A voxel grid over a cloud in the reference's (N,3) layout (additive to ABI 12; build-defined: the reference has nothing of the kind).
 *   cell       per axis floor((double)x / voxel), the origin fixed at 0; a cell must lie in [-2^20, 2^20)
 *   voxel ids  in first-occurrence order: first[v], voxel v's lowest point index, increases strictly with v
 *   centroid   (xyz and rgb alike) q = llrint((double)a * 65536) (half to even), S[v] = sum of q as exact int64,
 *              (float)((double)S / ((double)count * 65536.0)): integer sums, so the bits do not depend on the order of summation
 *   weight     w_i = 1 where count[cell_i] <= cap, else (float)((double)cap / (double)count[cell_i])
 * pcl_voxel_grid writes cell[n] (the voxel id of every point, in the caller's point order), count[v] and first[v] for v < *nvoxels (the
 * entries at and beyond *nvoxels of the n-entry buffers are not written) and *nvoxels (device int).  pcl_voxel_centroids writes
 * xyz_out / rgb_out, (nvoxels, 3) each, in voxel-id order; pcl_density_weights w[n].  A point whose cell[] lies outside [0, nvoxels) adds
 * nothing to a centroid and weighs 0.  *bad (device int, set by the call: 0 when all is well) is a bit set — 1: a value that is NaN or
 * infinite, 2: a cell outside +-2^20, 4: a magnitude >= 32768 (the grid looks at xyz, the centroids at xyz and rgb); with a bit set the
 * outputs hold valid indices but must not be used.  One workspace size serves both calls, pcl_voxel_workspace_bytes(n) (0 for n outside
 * 1..PCL_MAX_POINTS); the library initialises what it needs: results do not depend on what the workspace or the outputs held before.
 * PCL_EINVAL, before any HIP call: a null pointer, n outside 1..PCL_MAX_POINTS, voxel not positive and finite, nvoxels outside 1..n,
 * cap < 1.  PCL_EWORKSPACE: workspace_bytes below the query. */
size_t pcl_voxel_workspace_bytes(int64_t n);
int pcl_voxel_grid(const float *xyz, int64_t n, double voxel, int32_t *cell, int32_t *count, int64_t *first, int32_t *nvoxels, int32_t *bad,
                   void *workspace, size_t workspace_bytes, void *stream);
int pcl_voxel_centroids(const float *xyz, const float *rgb, int64_t n, const int32_t *cell, const int32_t *count, int64_t nvoxels, float *xyz_out,
                        float *rgb_out, int32_t *bad, void *workspace, size_t workspace_bytes, void *stream);
int pcl_density_weights(const int32_t *cell, const int32_t *count, int64_t n, int64_t nvoxels, int64_t cap, float *w, void *stream);
/* From the voxel grid to the cloud's up direction (additive to ABI 12; build-defined: the reference calls data_utils.obtain_align_matrix
 * and never defines it).  DESIGN.md section 2d.
 *   moments    (nvoxels, 9) int64, zeroed by the call.  q(a) = llrint((double)a * 65536), d_i = q(x_i) - q(x_first[v]) per axis;
 *              S1 = sum d (3), S2 = sum d_a d_b in the order xx xy xz yy yz zz: exact integers, the same bits for any launch shape.
 *              The sums are about the voxel's FIRST point, which the point order chooses: another order gives other moments and
 *              the same scatter matrix count S2 - S1 S1^T, exactly, hence the same normals.
 *              Range: points of one cell lie less than a voxel apart, |d| <= voxel 65536 + 1; at voxel <= 2 m d^2 < 2^34.0001 and
 *              PCL_MAX_POINTS = 2^27 of them stay below 2^63; a voxel above 2 m is refused.  `voxel` is the grid's.  A point with a bad
 *              coordinate (*bad as pcl_voxel_centroids sets it: 1 NaN or infinite, 4 magnitude >= 32768), one whose cell[] lies outside
 *              [0, nvoxels), and one whose voxel's first[] lies outside [0, n) or names a bad point, adds nothing.
 *   normals    A = count S2 - S1 S1^T exactly (128-bit integers), every entry rounded once to double and divided by
 *              ((double)count * (double)count * 2^32): the covariance in m^2.  Eigenvalues l0 <= l1 <= l2 by cyclic Jacobi in double
 *              (8 sweeps, contraction off).  normal (nvoxels, 3): the unit eigenvector of l0, its component of largest magnitude (the
 *              first of equals) positive; planarity = (l1 - l0) / l2; eig (nvoxels, 3) = (l0, l1, l2), or a null pointer.  A voxel with
 *              count < min_count or l2 <= 0 gets zeros.
 *   vote       w_v = count_v * llrint(planarity_v * 4096) (a voxel with planarity outside (0, 1], count <= 0 or a normal that is not a
 *              unit vector does not vote).  Up: the normals folded into z >= 0 and within max_tilt degrees of +z fill 64 x 64 int64 bins
 *              over (n_x / n_z, n_y / n_z) in [-tan max_tilt, tan max_tilt]^2; the heaviest bin (the lowest index of equals) starts the
 *              estimate; three rounds of e <- normalise(sum w_v llrint(n 2^20)) over the folded normals with n . e >= cos 5 degrees.
 *              Walls (params->yaw): the normals within 10 degrees of the horizontal plane after the up rotation; their azimuth modulo 90
 *              degrees fills 360 bins; within 3 degrees of the heaviest bin's centre sum w_v llrint(cos 4 psi 2^20), sum w_v llrint(sin 4 psi 2^20)
 *              name 4 phi, phi in (-45, 45] degrees.  rot = Rz(-phi) * (the minimal rotation taking up to +z): x_aligned = rot x.
 *              status 0; 1: no voxel inside the tilt cone, rot is the identity; 2: no wall normals, phi = 0.  weight[]: what the up bins, the
 *              last cone round, the wall bins and the wall mean kept.  All accumulation is in integers: one set of bits for any launch
 *              shape.  pcl_align_workspace_bytes(nvoxels) is one size for every count (0 outside 1..PCL_MAX_POINTS); the call initialises it.
 *   transform  out = R (x - a) in fp32, d = x - a, out_r = (R_r0 d_0 + R_r1 d_1) + R_r2 d_2, contraction off; rot (9) and trans (3)
 *              are device floats.  (pcl_transform_cloud below is the pose form: yaw / pitch / roll, the reference's operation order.)
 * PCL_EINVAL, before any HIP call: a null pointer (eig may be null), n outside 1..PCL_MAX_POINTS, nvoxels outside 1..n (moments) or
 * 1..PCL_MAX_POINTS, voxel not in (0, 2], min_count < 3, max_tilt not in (0, 45].  PCL_EWORKSPACE: workspace_bytes below the query. */
typedef struct pcl_align_params {
    double max_tilt;  /* degrees, in (0, 45] */
    int32_t yaw;      /* != 0: the wall direction too */
    int32_t reserved;
} PclAlignParams;
typedef struct pcl_align_out {
    double up[3];
    double rot[9];    /* row-major */
    double cos_tilt, sin_tilt, cos_yaw, sin_yaw;
    int64_t weight[4];
    int64_t status;
} PclAlignOut;
int pcl_voxel_moments(const float *xyz, int64_t n, double voxel, const int32_t *cell, const int64_t *first, int64_t nvoxels, int64_t *moments,
                      int32_t *bad, void *stream);
int pcl_voxel_normals(const int64_t *moments, const int32_t *count, int64_t nvoxels, int64_t min_count, float *normal, float *planarity,
                      float *eig, void *stream);
size_t pcl_align_workspace_bytes(int64_t nvoxels);
int pcl_align_vote(const float *normal, const float *planarity, const int32_t *count, int64_t nvoxels, const PclAlignParams *params,
                   PclAlignOut *out, void *workspace, size_t workspace_bytes, void *stream);
int pcl_align_transform_cloud(const float *xyz, int64_t n, const float *rot, const float *trans, float *out, void *stream);

size_t pcl_pano_bytes(int H, int W, int pano_format);
int pcl_pano_pack(const float *img_hwc, int H, int W, float *pano, void *stream);
int pcl_pano_pack_u8(const float *img_hwc, int H, int W, uint32_t *pano, int *not_exact, void *stream);
int pcl_pano_pack_u8p(const float *img_hwc, int H, int W, uint32_t *pano, int *not_exact, void *stream);
int pcl_pano_pack_u8v(const float *img_hwc, int H, int W, uint32_t *pano, int *not_exact, void *stream);
int pcl_pano_pack_f16(const float *img_hwc, int H, int W, void *pano, int *not_exact, void *stream);

/* ---- panorama pyramid (build-defined, additive to ABI 12: the reference resizes its query on the host to two fixed sizes and has no
 * pyramid).  Level 0 is the query image, every value exactly k/255.  Level l is made from level l - 1 — cascaded, never from level 0
 * directly — by ALIGNED 2 x 2 blocks in integer arithmetic on the levels k (aligned blocks: nothing wraps in azimuth; a plain box
 * pyramid: NO latitude weighting):
 *   - a pixel is BLACK when its three channels are 0: the loss's "no data" marker (mask = not (c == 0 on all three channels));
 *   - cnt = the non-black pixels of the block; cnt == 0: the output is black;
 *   - otherwise, per channel, k_out = (sum of k over the non-black pixels + cnt / 2) / cnt in integer division (round to nearest, ties up);
 *   - if that rounds every channel to 0, every channel whose sum equals the largest channel sum gets level 1 (the only reachable case:
 *     cnt == 3, sums 1, 1, 1) — so a coarse pixel is black iff there is no data under it;
 *   - a level's float value is the correctly rounded fp32 quotient k / 255 (as the pack kernels test it): every level is an exact-level
 *     image again and takes the F16 / U8 texel formats.
 * pcl_pano_pyramid_bytes: the bytes of the packed texels of levels 1..levels, level l in format formats[l - 1] (PCL_PANO_F16, _U8 or
 * _F32) at a 256-byte aligned offset, its region pcl_pano_bytes(H >> l, W >> l, format) rounded up to 256 bytes; 0 for anything refused:
 * levels outside 1..4, H or W not a multiple of 2^levels, another format, NULL.
 * pcl_pano_pyramid: ONE launch for all levels.  Writes every byte of `texels` (pcl_pano_pyramid_bytes of them) once: per level the
 * zero-bordered texels, byte for byte what the pack kernel of that format writes for the level's float image, and zeros up to the next
 * 256-byte boundary.  images (nullable): the float (H >> l, W >> l, 3) level images, level 1 first, one behind the other.  *not_exact
 * (device int, caller zeroes it) is set when a source value is not exactly k/255 — pcl_pano_pack_u8's pattern; the outputs are then
 * meaningless.  img_hwc must be 8-byte aligned (PCL_EINVAL otherwise). */
size_t pcl_pano_pyramid_bytes(int H, int W, int levels, const int *formats);
int pcl_pano_pyramid(const float *img_hwc, int H, int W, int levels, const int *formats, void *texels, float *images, int *not_exact,
                     void *stream);

/* ---- sampling loss (+ gradient) ----------------------------------------------------------------------------
 * Replaces SamplingLoss.forward (omniloc.py:171-202), BatchSamplingLoss.forward (omniloc.py:311-356), the forward
 * in trim_input_loss (utils.py:484-499) and sampling_loss (omniloc.py:105-157), plus — with with_grad != 0 — the
 * autograd backward the reference runs at omniloc.py:47,254, all fused in one pass over the cloud.
 *
 *   trans [B][3], rot [B][3] = (yaw, pitch, roll)
 *   result[B][PCL_RESULT_STRIDE] = loss, count, dL/dt(3), dL/d(yaw,pitch,roll)   (grad slots 0 if !with_grad)
 *   visible : nullable uint8 [B][n] in PACKED point order, multiplied into the mask (build-defined depth mask,
 *             off in the reference; see pcl_scatter_min_depth)
 * loss = sum_i mask_i ||c_i - rgb_i||_2 / sum_i mask_i, mask_i = sampled colour not exactly (0,0,0); 0/0 -> NaN.
 * Limits (32-bit buffer addressing): n <= 2^27 points, packed panorama < 2 GiB; PCL_EINVAL beyond.
 */
size_t pcl_loss_workspace_bytes(int64_t n, int B);
/* The same with the scatter-min depth mask OF THE SAME POSES multiplied into the mask (build-defined; see pcl_depth_mask below for
 * the definition): the z-buffers of the B poses are built on a depth_h x depth_w grid from every depth_stride-th point (0 x 0 / 0:
 * pcl_depth_default) and the loss kernel looks every point's cell up — what one depth-masked GD iteration evaluates.  Equal to
 * pcl_depth_mask on that grid / stride followed by pcl_sampling_loss(visible = that mask).  workspace: pcl_loss_depth_workspace_bytes
 * with the SAME depth_h / depth_w / depth_stride (the default grid depends on the stride; 0 for an invalid grid).  depth_stride 1, 2 and 4
 * have coalesced z passes; other strides (<= 64) are accepted and slower than reading every point.  depth_h, depth_w < 2^24. */
size_t pcl_loss_depth_workspace_bytes(int64_t n, int B, int H, int W, int depth_h, int depth_w, int depth_stride);
int pcl_sampling_loss_depth(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                            const float *rot, int B, int with_grad, int depth_h, int depth_w, float tau, int depth_stride, float *result,
                            void *workspace, size_t workspace_bytes, void *stream);
int pcl_sampling_loss(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans,
                      const float *rot, int B, int with_grad, const uint8_t *visible, float *result, void *workspace,
                      size_t workspace_bytes, void *stream);
/* pcl_sampling_loss over a cloud with per-point weights (`weights`: the plane of pcl_cloud_pack_weights; definitions above).  The same
 * launch plan as pcl_sampling_loss plus one plane; workspace: pcl_loss_workspace_bytes(n, B).  No byte mask, no depth mask. */
int pcl_sampling_loss_weighted(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W,
                               const float *trans, const float *rot, int B, int with_grad, float *result, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---- gradient-descent refinement ---------------------------------------------------------------------------
 * Replaces the optimisation loops of omniloc (omniloc.py:44-58) and omniloc_batch (omniloc.py:249-269): per
 * iteration one fused loss+gradient pass and one epilogue that does, per candidate and entirely on the device,
 * the final reduction, the chain rule to (t, yaw, pitch, roll), torch.optim.Adam (betas 0.9/0.999, eps 1e-8),
 * ReduceLROnPlateau(mode='min', threshold 1e-4 rel, cooldown 0, min_lr 0, eps 1e-8) and the clamp of t to `box`.
 *
 *   mode PCL_GD_SEQUENTIAL : clamp applies to the parameters the next forward sees          (omniloc.py:52-58)
 *   mode PCL_GD_BATCH      : the next forward sees the post-step PRE-clamp copy while Adam keeps updating the
 *                            clamped leaf (one-iteration lag of omniloc.py:260-269)
 *   box[6] = x_min, x_max, y_min, y_max, z_min, z_max  (device; quantile() of each xyz column, omniloc.py:53-55)
 *   state   : pcl_gd_state_bytes(B) bytes, opaque; pcl_gd_init fills it from the starting poses
 *   loss_history : nullable [num_iter][B]; loss of every forward
 * pcl_gd_run enqueues num_iter iterations back to back (no host synchronisation; capturable in a hipGraph) and may
 * be called repeatedly to continue.  pcl_gd_result writes, per candidate, PCL_GD_RESULT_STRIDE floats:
 *   fwd t(3), fwd ypr(3)  — the pose the reference returns (omniloc.py:102 / :272-275),
 *   leaf t(3), leaf ypr(3) — what the caller's input_trans/input_rot rows hold afterwards (omniloc.py:15-19,216-219),
 *   last loss (loss of the LAST forward, i.e. at the pose before the final update, omniloc.py:46,102,271,276), lr,
 *   ReduceLROnPlateau's num_bad_epochs and best (as floats; what the teacher-forced parity test compares with the reference's).
 */
#define PCL_GD_SEQUENTIAL 0
#define PCL_GD_BATCH 1
#define PCL_GD_RESULT_STRIDE 16

typedef struct pcl_gd_hyper {
    double lr;          /* cfg.lr        (omniloc.py:25)  */
    double factor;      /* cfg.factor    (omniloc.py:28)  */
    int32_t patience;   /* cfg.patience  (omniloc.py:27)  */
    int32_t mode;       /* PCL_GD_SEQUENTIAL | PCL_GD_BATCH */
    int32_t depth_mask; /* 0 = reference behaviour; 1 = the scatter-min depth mask of the poses each iteration evaluates multiplies
                           into the loss mask: before every loss pass the z-buffers of all B candidates are rebuilt (fill + z pass,
                           csrc/pcl_depth.hip) and the loss kernel looks each point's cell up (build-defined, cfg key `depth_mask`) */
    float depth_tau;    /* visibility tolerance: a point is visible iff its distance <= (1 + depth_tau) x the smallest distance in its cell */
    int32_t depth_h;    /* the z-buffer's grid (make_pano's pixel formula, utils.py:158-165, on depth_h x depth_w cells): chosen by point  */
    int32_t depth_w;    /* density, NOT the panorama's resolution.  0 x 0: pcl_depth_default(n, H, W, depth_stride).                         */
    int32_t depth_stride; /* the z-buffers are built from every depth_stride-th point of the packed cloud (every point is still TESTED       */
                        /* against them).  0: pcl_depth_default's choice with a default grid, 1 with a given grid.                           */
    int32_t fuse;          /* 0: pcl_gd_plan's rule (ONE launch per iteration when every block of the launch is resident at once).     */
                           /* < 0: never — always loss launch + epilogue launch.  Same bits either way (tests compare the two forms).  */
                           /* A chain of two launches per iteration without the depth mask, enqueued on a stream that is not capturing, */
                           /* runs as TWO half-chains over the two halves of its pose groups — the caller's stream and a side stream of */
                           /* the library, forked and joined by events inside the call: no host synchronisation, and whatever follows   */
                           /* on the caller's stream sees the finished state — when each half has at least 896 loss blocks (7/8 of what */
                           /* the GPU holds at once).  Every group runs under the whole chain's plan: same bits, split or not.  0 and   */
                           /* -1: that rule;                                                                                            */
                           /* -2: -1 and never split; -3: -1 and split whenever there are two pose groups (tests reach the path at      */
                           /* small sizes).  (pcl_gd_run, _run_weighted, _run_weight_sets; the rooms and depth chains never split.)     */
    int32_t images;        /* number of query images whose candidates share this launch chain (pcl_gd_set_panos / _set_pano_groups;   */
                           /* image i's candidates a contiguous range).  0 / 1: one image.  A hint for the block -> XCD mapping only    */
                           /* (with several panoramas every XCD takes a range of pose groups, i.e. of images, over the whole cloud      */
                           /* instead of a slice of the cloud for all of them): results do not depend on it.                            */
    int32_t color_sets;    /* 0 / 1: the cloud's one colour set.  k > 1: `cloud` holds k colour sets (pcl_cloud_pack_sets), the B candidates */
                           /* are k images of B / k (image i's a contiguous range) and image i's candidates read set i.  The chain then runs */
                           /* the SINGLE-IMAGE plan pcl_gd_plan(n, B / k) — its chunks, poses per block and steps per chunk — for all B: */
                           /* every image's results are those of a one-image run with its own colours, bit for bit.  pcl_gd_init writes */
                           /* the sets into the pose records; B % k != 0 or depth_mask: PCL_EINVAL (sizing functions: 0) — colour sets  */
                           /* under the depth mask run through pcl_gd_run_depth_chain.                                                 */
} pcl_gd_hyper;

size_t pcl_gd_state_bytes(int B);
/* workspace of pcl_gd_run: the loss partials, plus B z-buffers of depth_h x depth_w words when hyper->depth_mask is set (0 for an
 * invalid grid).  Pure scratch: every iteration refills what it reads, so a state may be continued with any workspace. */
size_t pcl_gd_workspace_bytes(int64_t n, int B, int H, int W, const pcl_gd_hyper *hyper_host);
int pcl_gd_init(void *state, const float *trans, const float *rot, int B, const pcl_gd_hyper *hyper_host, void *stream);
int pcl_gd_run(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, void *state, int B, const float *box,
               const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace,
               size_t workspace_bytes, void *timer, void *stream);
/* pcl_gd_run over a cloud with per-point weights (`weights`: the plane of pcl_cloud_pack_weights).  State, workspace
 * (pcl_gd_workspace_bytes), pcl_gd_init / _result / _winner / _set_pano_groups and pcl_gd_plan are pcl_gd_run's: the same chunks, poses
 * per block and fuse rule (hyper->fuse), one more plane per loss block, capturable alike.  PCL_EINVAL with hyper->depth_mask or
 * hyper->color_sets > 1. */
int pcl_gd_run_weighted(const float *cloud, const float *weights, int64_t n, const void *pano, int pano_format, int H, int W, void *state, int B,
                        const float *box, const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace,
                        size_t workspace_bytes, void *timer, void *stream);
/* One weight plane per query image (additive to ABI 12): pcl_gd_run_weighted for a chain whose B candidates are nsets images of B / nsets
 * (image i's a contiguous range, its panorama named by pcl_gd_set_pano_groups), image i's candidates reading plane i of `weights`: nsets
 * planes of pcl_cloud_stride(n) floats, plane i behind plane i - 1.  weights == NULL: the unweighted loss.  Either way the chain runs the
 * SINGLE-IMAGE plan pcl_gd_plan(n, B / nsets) — its chunks, poses per block and steps per chunk — for all B candidates, with shared colours
 * (hyper->color_sets 0 / 1) as with per-image colour sets (hyper->color_sets == nsets, pcl_cloud_pack_sets), so image i's state, pose records
 * and loss-history columns equal those of pcl_gd_run / pcl_gd_run_weighted of that image alone with plane i, BIT FOR BIT, fused or two
 * launches (hyper->fuse: the same rule over all blocks), eager or replayed.  A block finds its plane through `cset` of its group's first
 * pose record: pcl_gd_init_weight_sets (pcl_gd_init for this layout) writes cset = b / (B / nsets) into both copies of the records, with
 * shared colours too.  State, pcl_gd_result / _winner / _set_pano_groups as for pcl_gd_run; workspace pcl_gd_weight_sets_workspace_bytes;
 * pcl_gd_plan_weight_sets is pcl_gd_plan for this chain (host-only, outputs nullable).  The robust chain over several images: run
 * unweighted, pcl_gd_winner -> pcl_point_residuals_images -> pcl_robust_weights_rows into the planes, run on with them.
 * PCL_EINVAL (0 from the size query), before any HIP call: nsets < 1, B % nsets != 0, hyper->color_sets > 1 that is not nsets,
 * hyper->depth_mask, a candidate count per image that the plan's poses per block do not divide, n outside 1..PCL_MAX_POINTS, and what
 * pcl_gd_run refuses.  PCL_EWORKSPACE: workspace_bytes too small. */
size_t pcl_gd_weight_sets_workspace_bytes(int64_t n, int B, int nsets, const pcl_gd_hyper *hyper_host);
int pcl_gd_plan_weight_sets(int64_t n, int B, int nsets, const pcl_gd_hyper *hyper_host, int *nchunks_host, int *poses_per_block_host, int *fused_host);
int pcl_gd_init_weight_sets(void *state, const float *trans, const float *rot, int B, int nsets, const pcl_gd_hyper *hyper_host, void *stream);
int pcl_gd_run_weight_sets(const float *cloud, const float *weights, int nsets, int64_t n, const void *pano, int pano_format, int H, int W, void *state,
                           int B, const float *box, const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace,
                           size_t workspace_bytes, void *timer, void *stream);
int pcl_gd_result(const void *state, int B, float *result, void *stream);
/* Teacher-forcing hook (parity tests): ONE optimiser step of every candidate from a GIVEN loss [B] and
 * gradient [B][6] = dL/d(t0, t1, t2, yaw, pitch, roll) — e.g. the reference's recorded loss_list and autograd gradients
 * (omniloc.py:253-254) — through the very update code of pcl_gd_run's epilogue: torch.optim.Adam, ReduceLROnPlateau, the clamp to
 * `box` in the given mode, the next forward pose.  Updates `state` in place (copy 0: follow with pcl_gd_result); scratch: B * 8
 * floats.  last loss / lr / the scheduler's counters advance exactly as in a run. */
int pcl_gd_step_from_grads(void *state, int B, const float *loss, const float *grad, const float *box, const pcl_gd_hyper *hyper_host,
                           float *scratch, void *stream);
/* How pcl_gd_run decomposes an n-point, B-candidate problem (host-only query, measurement aid): chunks of the cloud, poses per
 * block, and whether an iteration is ONE launch (the loss launch of iteration k + 1 finishes iteration k in the prologue of every
 * block: launches whose chunk x group blocks are all resident at once — the reference's shipped 167k-point / 6-candidate shape)
 * or two (loss + epilogue).  Any of the three outputs may be NULL. */
int pcl_gd_plan(int64_t n, int B, int *nchunks_host, int *poses_per_block_host, int *fused_host);
/* the same for the hyper-parameters a run will use: a depth-masked run (hyper->depth_mask) never fuses; hyper NULL = pcl_gd_plan */
int pcl_gd_plan_hyper(int64_t n, int B, const pcl_gd_hyper *hyper_host, int *nchunks_host, int *poses_per_block_host, int *fused_host);
/* Several query images against one shared cloud in ONE launch chain (BASELINE cfg 4: independent panoramas, shared
 * cloud): candidate b samples panos[b] (device array of B device addresses of packed panoramas; all the same H, W and
 * texel format as the `pano` passed to pcl_gd_run, which stays the default for entries that are 0).  Call after
 * pcl_gd_init (which resets every candidate to the default panorama); panos == NULL clears the table.  More poses per
 * launch share each cloud chunk in L2 and amortise the per-block costs: at cfg 2, 4 images x 32 candidates per launch
 * run at the efficiency of cfg 3. */
int pcl_gd_set_panos(void *state, const uint64_t *panos, int B, void *stream);
/* The same from a short HOST list: candidates [i * per_image, (i + 1) * per_image) sample panos_host[i] (device addresses of
 * packed panoramas; B = nimages * per_image).  The addresses travel as kernel arguments — nothing is copied to the device, so
 * nothing waits for the work the stream already holds (one launch per 64 images). */
int pcl_gd_set_pano_groups(void *state, const uint64_t *panos_host, int nimages, int per_image, void *stream);
/* The plateau scheduler starts over (additive to ABI 12; one small launch): in both copies of the state, `best` and `num_bad` of every
 * candidate become what pcl_gd_init writes (+inf, 0).  Every other byte stays: lr, Adam's moments, the step count, the pose records.
 * For a chain that goes on against another panorama level (pcl_pano_pyramid), whose losses do not compare with the last level's. */
int pcl_gd_plateau_reset(void *state, int B, void *stream);
/* The end of omniloc_batch, omniloc.py:271-277, for nimages x per_image candidates (B = nimages * per_image): per image the
 * candidate whose LAST forward had the smallest loss (torch.argmin semantics: first of equal minima, a NaN loss wins), as
 * winners [nimages][16] = post-step translation (3), R = RZ(yaw) RY(pitch) RX(roll) of the post-step angles (9, row-major),
 * that loss, yaw / pitch / roll.  leaf_trans / leaf_rot [B][3] (nullable) receive every candidate's leaf parameters — what the
 * reference leaves in the caller's input_trans / input_rot, whose rows it optimises in place (omniloc.py:216-219). */
int pcl_gd_winner(const void *state, int nimages, int per_image, float *winners, float *leaf_trans, float *leaf_rot, void *stream);
/* Prune a GD state on the device (additive to ABI 12): per group keep the `keep` best candidates by their last loss and hand their COMPLETE
 * optimiser state to a smaller state, so that a chain goes on with fewer candidates without a host round trip.  `state_in`: a state of
 * groups * per_group candidates as pcl_gd_init / any pcl_gd_run* call leaves it (copy 0 is current); group g is the contiguous candidates
 * [g * per_group, (g + 1) * per_group) — an image of pcl_gd_run, a (room, image) of the rooms chains.  `state_out`: a distinct buffer of
 * pcl_gd_state_bytes(groups * keep).  Order: pcl_gd_winner's (a NaN is ahead of every number; among equal losses, or among NaNs, the
 * smaller index is ahead; -0.0 == +0.0); a group keeps the candidates that `keep` successive "take the winner, remove it" steps would take,
 * so keep = 1 keeps exactly the candidate pcl_gd_winner names.  Survivors keep their ORIGINAL index order: slot g * keep + s holds group
 * g's s-th survivor and survivors[g * keep + s] its index inside the group (0 .. per_group - 1).  Copied, nothing recomputed: the
 * survivor's whole optimiser record (Adam moments, lr, scheduler best / bad epochs, step, bias-correction products, sin / cos) and its
 * pose record of BOTH copies (pose, panorama address, colour set) — bit for bit what pcl_gd_init + pcl_gd_set_panos* + the run would have
 * left for those candidates alone.  leaf_trans / leaf_rot [groups * per_group][3] (nullable) receive every INPUT candidate's leaf
 * parameters, as pcl_gd_winner writes them.  keep == per_group is a plain copy.  One launch of one 256-thread block per group, no
 * workspace, no atomics; capturable.
 * PCL_EINVAL, before any HIP call: null state_in / state_out / survivors, state_out == state_in, a state that is not 16-byte aligned,
 * groups <= 0, keep <= 0, keep > per_group, per_group > PCL_GD_PRUNE_MAX, groups * per_group above 2^30. */
#define PCL_GD_PRUNE_MAX 1024 /* candidates per group */
int pcl_gd_prune(const void *state_in, int groups, int per_group, int keep, void *state_out, int32_t *survivors, float *leaf_trans,
                 float *leaf_rot, void *stream);

/* Room search (ABI 11): ONE query panorama against the rooms of a building in ONE launch chain.  Room r's candidates are the contiguous
 * range [r * per_room, (r + 1) * per_room) of a state of B = nrooms * per_room candidates (pcl_gd_state_bytes / pcl_gd_init /
 * pcl_gd_result as for pcl_gd_run; pcl_gd_winner(state, nrooms, per_room, ...) gives one winner per room), all sampling `pano`.
 * Every room keeps its own cloud (packed by pcl_cloud_pack), its own clamp box and its own decomposition: room r's loss blocks run
 * pcl_gd_plan(n_r, per_room)'s chunks, poses per block and steps per chunk over its own cloud, and its candidates are finished from its
 * own partial sums in the same order as there.  Contract: each room's results — state, pose records, loss history columns — equal those
 * of a pcl_gd_run of that room alone (same per_room candidates, same hyper-parameters) BIT FOR BIT, fused or not, eager or replayed.
 * The room table is written to device memory by one small launch at the start of every pcl_gd_run_rooms call (its values travel as
 * kernel arguments: no host-to-device copy), so a call stays capturable in a hipGraph.  An iteration is one launch when the blocks of
 * all rooms together fit the fuse rule of pcl_gd_plan (hyper->fuse < 0: never), else two.
 * PCL_EINVAL (0 from the sizing function): nrooms outside 1..PCL_GD_MAX_ROOMS, per_room <= 0, a room with a null cloud or box or
 * n outside 1..PCL_MAX_POINTS, hyper->depth_mask, hyper->color_sets > 1, null arguments.  hyper->images is ignored (one panorama). */
#define PCL_GD_MAX_ROOMS 32
typedef struct pcl_gd_room {
    const float *cloud; /* packed cloud (pcl_cloud_pack) */
    int64_t n;          /* its points */
    const float *box;   /* device box[6] of the room (see pcl_gd_run) */
} pcl_gd_room;
size_t pcl_gd_rooms_workspace_bytes(const pcl_gd_room *rooms_host, int nrooms, int per_room, const pcl_gd_hyper *hyper_host);
/* host-only: per room the chunks of its plan (nchunks_host[nrooms], nullable), the poses per block (the same for all rooms), whether
 * an iteration is one launch */
int pcl_gd_plan_rooms(const pcl_gd_room *rooms_host, int nrooms, int per_room, const pcl_gd_hyper *hyper_host, int *nchunks_host,
                      int *poses_per_block_host, int *fused_host);
int pcl_gd_run_rooms(const pcl_gd_room *rooms_host, int nrooms, const void *pano, int pano_format, int H, int W, void *state, int per_room,
                     const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace, size_t workspace_bytes, void *timer,
                     void *stream);

/* Room search over several panoramas (ABI 12): nimages query panoramas x nrooms rooms x per_image candidates in ONE launch chain.
 * Candidate (r, i, j) is record (r * nimages + i) * per_image + j of a state of B = nrooms * nimages * per_image candidates
 * (pcl_gd_state_bytes / pcl_gd_result as for pcl_gd_run; pcl_gd_winner(state, nrooms * nimages, per_image, ...) gives one winner per
 * (room, image)).  Image i's panorama travels in its candidates' pose records: pcl_gd_set_pano_groups with the nrooms * nimages
 * addresses pano[i] repeated room by room; `pano` is the default for records that name none.  hyper->color_sets 0 / 1: the images share
 * room r's colours (pcl_cloud_pack); hyper->color_sets == nimages: every room's cloud holds one set per image (pcl_cloud_pack_sets with
 * nimages sets) and candidate (r, i, .) reads set i of room r — pcl_gd_init_rooms_images writes that into the pose records (it is
 * pcl_gd_init for this layout; pcl_gd_init itself would number the sets through the rooms).
 * Room r runs the SINGLE-IMAGE plan pcl_gd_plan(n_r, per_image) — chunks, poses per block, steps per chunk — for all nimages * per_image of
 * its candidates, with shared colours too, and a group of poses never straddles two images.  Contract: for every (r, i) the state, pose
 * records and loss-history columns equal those of a pcl_gd_run of room r with image i alone (per_image candidates, image i's colours, same
 * hyper-parameters) BIT FOR BIT — fused or two launches, eager or replayed, both modes, every nrooms >= 1 and nimages >= 1.
 * An iteration is one launch when the blocks of all rooms and images together fit the fuse rule (hyper->fuse < 0: never), else two; the
 * room table is written by one small launch from kernel arguments, so a call stays capturable.  nimages == 1 is pcl_gd_run_rooms.
 * PCL_EINVAL (0 from the sizing function), before any HIP call: null arguments, hyper->depth_mask, nrooms outside 1..PCL_GD_MAX_ROOMS,
 * nimages < 1, per_image < 1, hyper->color_sets other than 0, 1 or nimages, a room with a null cloud or box or n outside
 * 1..PCL_MAX_POINTS, a room whose cloud of nimages sets passes 2^31 bytes (pcl_cloud_sets_bytes answers 0: the caller groups its images).
 * PCL_EWORKSPACE: workspace_bytes below pcl_gd_rooms_images_workspace_bytes. */
size_t pcl_gd_rooms_images_workspace_bytes(const pcl_gd_room *rooms_host, int nrooms, int nimages, int per_image, const pcl_gd_hyper *hyper_host);
/* host-only: as pcl_gd_plan_rooms */
int pcl_gd_plan_rooms_images(const pcl_gd_room *rooms_host, int nrooms, int nimages, int per_image, const pcl_gd_hyper *hyper_host,
                             int *nchunks_host, int *poses_per_block_host, int *fused_host);
int pcl_gd_init_rooms_images(void *state, const float *trans, const float *rot, int nrooms, int nimages, int per_image,
                             const pcl_gd_hyper *hyper_host, void *stream);
int pcl_gd_run_rooms_images(const pcl_gd_room *rooms_host, int nrooms, int nimages, const void *pano, int pano_format, int H, int W, void *state,
                            int per_image, const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace,
                            size_t workspace_bytes, void *timer, void *stream);
/* pcl_pose_information and pcl_gn_refine for the nrooms * nimages winners of a rooms x images chain, in ONE set of launches (additive to
 * ABI 12; BUILD-DEFINED).  Pose (r, i) is row r * nimages + i of trans / rot — the layout of pcl_gd_winner(state, nrooms * nimages,
 * per_image, ...), so pose_stride 16 with trans = winners, rot = winners + 13 reads the winners in place — and is evaluated against room
 * r's packed cloud rooms_host[r].cloud of rooms_host[r].n points (pcl_gd_room.box is ignored and may be null), against panos_host[i] (HOST
 * array of nimages device addresses of packed panoramas of one H, W and texel format, as for pcl_pose_information_images) and against
 * colour set i of room r when color_sets == nimages (every room's cloud is then one of pcl_cloud_pack_sets with nimages sets; color_sets
 * 0 / 1: the room's one set).  No weights: the rooms chains take none.
 * Record (r, i) — info, cov; for pcl_gn_refine_rooms also out, the state (pcl_gn_state_bytes(nrooms * nimages)) and the trace rows
 * [iters + 1][nrooms * nimages][16] — equals what pcl_pose_information / pcl_gn_refine returns for that pose against room r's cloud, that
 * colour set and panos_host[i] alone, in the same texel format, BIT FOR BIT, for every nrooms >= 1 and nimages >= 1: room r walks its own
 * chunking (that of the single call: it depends on n_r alone) into its own region of partial rows, and a pose is finished over its room's
 * rows by the code of the single call.  A frozen pose stops only its own blocks.  The room records (cloud address, n, stride, chunks,
 * steps, first block, row offset) and the panorama addresses travel as kernel arguments: nothing is copied, nothing waits for the host,
 * capturable.  Per evaluation one pass launch per 64 images (all rooms in each; colour set and row are counted from the call's first
 * image) and one step launch over all poses; pcl_pose_information_rooms: the pass launches and one finish launch.  No atomics, no
 * allocation, no synchronisation.  workspace: the sum over the rooms of pcl_pose_information_workspace_bytes(n_r, nimages).
 * PCL_EINVAL (0 from the sizing functions, for what they are told), before any HIP call: everything pcl_pose_information_images /
 * pcl_gn_refine_images refuse (B = nimages; no weights); nrooms outside 1..PCL_GD_MAX_ROOMS; a room with a null cloud or n outside
 * 1..PCL_MAX_POINTS; a room whose colour sets pass 2^31 bytes (one buffer resource per room); more blocks than a grid holds; a workspace
 * below the query.
 * Deliberately left out: the depth chains, weights (the rooms chains have none), and any claim that cov is calibrated on real data. */
size_t pcl_pose_information_rooms_workspace_bytes(const pcl_gd_room *rooms_host, int nrooms, int nimages);
int pcl_pose_information_rooms(const pcl_gd_room *rooms_host, int nrooms, int color_sets, const uint64_t *panos_host, int nimages, int pano_format,
                               int H, int W, const float *trans, const float *rot, int pose_stride, float *info, float *cov, void *workspace,
                               size_t workspace_bytes, void *stream);
size_t pcl_gn_rooms_workspace_bytes(const pcl_gd_room *rooms_host, int nrooms, int nimages);
int pcl_gn_refine_rooms(const pcl_gd_room *rooms_host, int nrooms, int color_sets, const uint64_t *panos_host, int nimages, int pano_format, int H,
                        int W, const float *trans, const float *rot, int pose_stride, const pcl_gn_hyper *hyper_host, int iters, void *state,
                        float *out, float *info, float *cov, float *trace, void *workspace, size_t workspace_bytes, void *stream);

/* The depth mask inside a shared chain (additive to ABI 12): the rooms x images chain above with hyper->depth_mask set — which every
 * entry point above refuses, because this chain's workspace carries z-buffers.  One family for the three shared chains: per-image colour
 * sets of one room (nrooms = 1, color_sets = nimages), several rooms (nimages = 1), rooms x images.  Layout, state, panoramas and colour
 * sets as for pcl_gd_run_rooms_images: pcl_gd_state_bytes, pcl_gd_init_rooms_images (nrooms = 1 included; it does not read depth_mask),
 * pcl_gd_set_pano_groups, pcl_gd_result / pcl_gd_winner.  hyper->depth_mask must be set (else PCL_EINVAL; 0 from the sizing function).
 * Room r runs the single-image plan pcl_gd_plan(n_r, per_image) for all its candidates (two launches per iteration: a depth-masked run
 * never fuses) and resolves ITS OWN grid, tolerance and occluder stride from hyper->depth_h / depth_w / depth_tau / depth_stride exactly
 * as a pcl_gd_run of that room does: pcl_depth_default(n_r, H, W, depth_stride) for a 0 x 0 grid, the given grid for every room otherwise.
 * Per iteration: one z pass per room (its cloud, its candidates, its region of z-buffer set it & 1), ONE loss launch over all rooms that
 * looks every point's cell up in its room's z-buffers and resets the other set, ONE epilogue launch.  Contract: for every (r, i) the
 * state, pose records, loss-history columns and winner equal those of a depth-masked pcl_gd_run of room r with image i alone (image i's
 * colours, per_image candidates, the same hyper-parameters) BIT FOR BIT, in both modes, also across repeated calls.
 * workspace: room table, depth table, one partials buffer, two z-buffer sets (per set every room's nimages * per_image z-buffers); pure
 * scratch, every call fills the set its first iteration reads.  nrooms == 1 with nimages == 1 is pcl_gd_run itself.
 * PCL_EINVAL, before any HIP call: null arguments, depth_mask == 0, what pcl_gd_run_rooms_images refuses, an invalid grid (a side below
 * 2, one side 0), a room whose nimages * per_image z-buffers reach 4 GiB.  PCL_EWORKSPACE: workspace_bytes too small.
 * pcl_gd_plan_depth_chain (host-only; every output nullable): per room the chunks of its plan, grid and occluder stride; poses per block. */
size_t pcl_gd_depth_chain_workspace_bytes(const pcl_gd_room *rooms_host, int nrooms, int nimages, int per_image, int H, int W,
                                          const pcl_gd_hyper *hyper_host);
int pcl_gd_plan_depth_chain(const pcl_gd_room *rooms_host, int nrooms, int nimages, int per_image, int H, int W, const pcl_gd_hyper *hyper_host,
                            int *nchunks_host, int *poses_per_block_host, int *depth_h_host, int *depth_w_host, int *depth_stride_host);
int pcl_gd_run_depth_chain(const pcl_gd_room *rooms_host, int nrooms, int nimages, const void *pano, int pano_format, int H, int W, void *state,
                           int per_image, const pcl_gd_hyper *hyper_host, int num_iter, float *loss_history, void *workspace,
                           size_t workspace_bytes, void *timer, void *stream);

/* ---- kernel timer (measurement aid, HOST object) --------------------------------------------------------------
 * A pool of hipEvent pairs.  When a timer is passed to pcl_gd_run, every launch of the fused loss+gradient kernel is
 * bracketed by an event pair recorded on `stream` (no synchronisation inside the run).  pcl_timer_read synchronises
 * on the recorded events and returns the summed kernel time and the number of launches since the last reset.
 * Launches beyond `capacity` are simply not timed. */
void *pcl_timer_create(int capacity);
void pcl_timer_destroy(void *timer);
void pcl_timer_reset(void *timer);
void pcl_timer_set_stride(void *timer, int stride); /* time only every stride-th launch of a run (default 1) */
int pcl_timer_read(void *timer, double *total_ms_host, int *launches_host);
/* What an event pair reads with NOTHING between its two records: `reps` empty pairs are recorded on `stream`, the call
 * synchronises on them and returns their median elapsed time (ms).  A pair around a kernel over-reads the kernel's duration
 * by about this much (the two event packets' own processing); bench.py subtracts it per timed launch.  Uses its own events,
 * leaves the timer's recorded pairs untouched. */
int pcl_timer_calibrate(void *timer, int reps, double *pair_ms_host, void *stream);

/* ---- stand-alone ops of the path ---------------------------------------------------------------------------- */
/* utils.py:16-61 cloud2idx: xyz [n][3] -> coord [n][2] in [-1,1]^2 (batched form = same call on B*n points). */
int pcl_cloud2idx(const float *xyz, int64_t n, float *coord, void *stream);
/* utils.py:64-103 sample_from_img: clip to +-0.99, bilinear, zero padding, align_corners=False; rgb_out [n][3]. */
int pcl_sample_from_img(const void *pano, int pano_format, int H, int W, const float *coord, int64_t n, float *rgb_out,
                        void *stream);
/* Backward of the two ops above, for callers that differentiate through them outside SamplingLoss (the reference's are plain
 * autograd ops, utils.py:16-103):
 *   pcl_cloud2idx_backward        grad_xyz [n][3] = J^T grad_coord [n][2]  (atan2 / norm chain rule of utils.py:44-59)
 *   pcl_sample_from_img_backward  grad_coord [n][2] (through torch.clip and grid_sampler_2d, utils.py:96-98; nullable) and
 *                                 grad_img [H][W][3] fp32, ACCUMULATED with float atomics into a caller-zeroed buffer
 *                                 (nullable); grad_rgb [n][3] is the incoming gradient. */
int pcl_cloud2idx_backward(const float *xyz, const float *grad_coord, int64_t n, float *grad_xyz, void *stream);
int pcl_sample_from_img_backward(const void *pano, int pano_format, int H, int W, const float *coord, const float *grad_rgb,
                                 int64_t n, float *grad_coord, float *grad_img, void *stream);
/* utils.py:425-453 rot_from_ypr for B poses: rot [B][3] -> R [B][9] row-major. */
int pcl_rot_from_ypr(const float *rot, int B, float *R, void *stream);
/* utils.py:208-229 quantile on each of the 3 columns of xyz [n][3]: box[6] = x[int(n q)], x[int(n (1-q))], y.., z..
 * (exact order statistics by radix select; workspace pcl_quantile_workspace_bytes()). */
size_t pcl_quantile_workspace_bytes(void);
int pcl_quantile_box(const float *xyz, int64_t n, double q, float *box, void *workspace, void *stream);

/* Build-defined scatter-min visibility (the reference imports torch_scatter.scatter_min at utils.py:6 but never
 * calls it).  For camera-frame points xyz_cam [n][3]: pixel = make_pano's (utils.py:158-165), depth = ||p||
 * (utils.py:152); zbuf [H*W] uint64 = min over the pixel of (depth_bits << 32 | index), 0xFFFF... if empty.
 * pcl_scatter_min_unpack turns it into torch_scatter's (out, arg) convention: empty -> (0, n). */
int pcl_scatter_min_depth(const float *xyz_cam, int64_t n, int H, int W, uint64_t *zbuf, void *stream);
int pcl_scatter_min_unpack(const uint64_t *zbuf, int64_t n, int H, int W, float *zmin, int64_t *argmin, void *stream);
/* utils.py:134-205 make_pano: 3x3 splat, nearest point wins inside a pass, later passes overwrite earlier ones
 * (order idx8..idx1, centre; utils.py:190-198).  image [H][W][3] float = rgb*255 (0 where nothing projects).
 * workspace: H*W uint64. */
int pcl_make_pano(const float *xyz_cam, const float *rgb, int64_t n, int H, int W, float *image, uint64_t *workspace,
                  void *stream);
/* Second trimming stage of the initialisation for a batch of candidate poses (utils.py:510-588 with
 * color_utils.py:68-144): render the packed world-frame cloud (pcl_cloud_pack) from every candidate (make_pano semantics
 * at the image's resolution; among points at exactly equal distance the larger PACKED index wins), and per block j of the middle block rows (h = 1 + j / nsw in 1..nsh-2, w = j % nsw) intersect the
 * normalised 8x8x8 colour histogram of the rendered pixels (both render and query non-black) with that of the query
 * image's non-black pixels.  inter [ncand][(nsh-2)*nsw], nproj [ncand][..] = pixels histogrammed, nimg [..] likewise
 * for the query.  The caller forms score = sum_j inter / (nsh*nsw) with the reference's empty-block rule. */
size_t pcl_hist_trim_workspace_bytes(int ncand, int H, int W, int nsh, int nsw);
/* Same for a cloud of n points, large enough for the tile-binned render (ABI v4): every candidate's points are binned by the
 * 64 x 64-pixel image tile(s) their 3 x 3 splat touches and every tile is resolved and histogrammed in LDS — no z-buffer in
 * HBM, bit-identical scores.  pcl_hist_trim_scores takes that path when its workspace is at least this large (4 n list
 * entries of 12 bytes per candidate: the exact worst case; plus the tiles' run tables, 8 bytes x tiles x ceil(n / 2048) per candidate)
 * and the z-buffer splat otherwise. */
size_t pcl_hist_trim_workspace_bytes_n(int64_t n, int ncand, int H, int W, int nsh, int nsw);
int pcl_hist_trim_scores(const float *cloud, int64_t n, const float *img_hwc, int H, int W, const float *trans,
                         const float *rot, int ncand, int nsh, int nsw, float *inter, int32_t *nproj, int32_t *nimg,
                         void *workspace, size_t workspace_bytes, void *stream);
/* score[cand] of the trimming stage from pcl_hist_trim_scores' outputs: sum of the block intersections of every block row
 * up to its first empty block (utils.py:568-571), divided by nsh * nsw (utils.py:580). */
int pcl_hist_trim_reduce(const float *inter, const int32_t *nproj, const int32_t *nimg, int ncand, int nsh, int nsw, float *score,
                         void *stream);
/* The same for `nimages` query images of ONE room in one set of launches (<= 32 images): candidates [i * cand_per_image,
 * (i + 1) * cand_per_image) of trans / rot are rendered and scored against imgs_host[i] (HOST array of device addresses of (H, W, 3)
 * float images); inter / nproj [nimages * cand_per_image][nblk], nimg [nimages][nblk], score [nimages * cand_per_image].  Every image's
 * candidates form their own chain of the empty-block carry-over (one call of the reference's function per image); results are
 * those of the single-image entry points, bit for bit. */
size_t pcl_hist_trim_images_workspace_bytes(int64_t n, int nimages, int cand_per_image, int H, int W, int nsh, int nsw);
int pcl_hist_trim_scores_images(const float *cloud, int64_t n, const float *const *imgs_host, int nimages, int cand_per_image, int H, int W,
                                const float *trans, const float *rot, int nsh, int nsw, float *inter, int32_t *nproj, int32_t *nimg,
                                void *workspace, size_t workspace_bytes, void *stream);
/* The same over a cloud of `color_sets` colour sets (pcl_cloud_pack_sets): color_sets == nimages renders image i's candidates with set i,
 * color_sets == 1 is pcl_hist_trim_scores_images.  The workspace of the tile-binned path holds one row of colour codes per set (size it
 * with the same color_sets; the size for n = 0 selects the z-buffer splat path). */
size_t pcl_hist_trim_images_sets_workspace_bytes(int64_t n, int color_sets, int nimages, int cand_per_image, int H, int W, int nsh, int nsw);
int pcl_hist_trim_scores_images_sets(const float *cloud, int64_t n, int color_sets, const float *const *imgs_host, int nimages, int cand_per_image,
                                     int H, int W, const float *trans, const float *rot, int nsh, int nsw, float *inter, int32_t *nproj,
                                     int32_t *nimg, void *workspace, size_t workspace_bytes, void *stream);
int pcl_hist_trim_reduce_images(const float *inter, const int32_t *nproj, const int32_t *nimg, int nimages, int cand_per_image, int nsh,
                                int nsw, float *score, void *stream);
/* First trimming stage of the initialisation, utils.py:462-507 trim_input_loss: the forward-only sampling loss
 * (utils.py:484-499 = omniloc.py:171-202 without gradient) of ALL K x R pairs of trans [K][3] and rot [R][3] (yaw, pitch, roll),
 * loss_table [K][R] row-major like the reference's `loss_table[i, j]` (utils.py:497; its argsort / index decode stay with the
 * caller), count_table [K][R] (nullable) = points kept by the mask.  Rotations that differ only in YAW share the projection:
 * with q' = RY(pitch) RX(roll) (x - t), theta does not depend on yaw and phi = atan2(q'_y, q'_x) + yaw - 1e-6 p_y / rho^2 (first
 * order in the reference's `x + 1e-6`; points within 0.1 mm of the camera's vertical axis are evaluated exactly), so a block
 * rotates a point and takes both atan2s once for up to four yaws.
 *   pcl_trim_groups: classes of equal (pitch, roll) of the rotation table (bitwise), built on the device into
 *     `groups` (pcl_trim_groups_bytes(R) bytes; its first int32 is the number of 4-yaw groups, which a caller may read back ONCE
 *     per rotation grid and pass as `ngroups`; passing R is always valid: surplus blocks return at once).
 *     R <= 1024 (PCL_EINVAL beyond: callers fall back to pcl_sampling_loss over the K x R pairs, as piccolo_amd/utils.py does).
 *   pcl_trim_loss: workspace pcl_trim_loss_workspace_bytes(n, K, ngroups).  The table is filled with NaN first; if `groups` was
 *     built from a table of another size, or holds more groups than `ngroups`, NOTHING is written over them: an entry the
 *     launch did not compute ranks last in the caller's selection (NaN), never as stale memory. */
size_t pcl_trim_groups_bytes(int R);
/* The two selections of the initialisation stage in one launch each (one block per problem, nprob problems of M values):
 *   largest == 0, rot_per_trans == len(rot):  utils.py:500-505  min_inds = loss_table.flatten().argsort()[:n_keep];
 *                                             out_trans = trans[min_inds // len(rot)], out_rot = rot[min_inds % len(rot)]
 *   largest == 1, rot_per_trans == 0:         utils.py:583-586  min_inds = flip(hist_intersect.argsort()[-n_keep:]);
 *                                             out_trans = trans[min_inds], out_rot = rot[min_inds]
 * values [nprob][M]; problem p reads its pose rows from trans / rot + p * pose_stride * 3 floats (pose_stride 0: shared tables);
 * out_trans / out_rot [nprob][n_keep][3], out_idx [nprob][n_keep] (nullable).  Exact and deterministic: ascending by value with
 * ties by ascending index (a stable argsort); largest: descending, ties by descending index (the flipped tail of that argsort);
 * NaN ranks last in both.  n_keep <= min(M, 1024). */
int pcl_select_poses(const float *values, int nprob, int M, int n_keep, int largest, const float *trans, const float *rot,
                     int rot_per_trans, int64_t pose_stride, float *out_trans, float *out_rot, int *out_idx, void *stream);
int pcl_trim_groups(const float *rot, int R, void *groups, void *stream);
size_t pcl_trim_loss_workspace_bytes(int64_t n, int K, int ngroups);
int pcl_trim_loss(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans, int K,
                  const float *rot, int R, const void *groups, int ngroups, const void *order, float *loss_table, float *count_table,
                  void *workspace, size_t workspace_bytes, void *stream);
/* The launch's WORK LIST (ABI 9; `order`, nullable, of pcl_trim_loss / pcl_trim_loss_images).  Which block evaluates which (cloud chunk,
 * (translation, rotation class) slot) item is scheduling only — every item's partial sum has its own place, the tables are bit-identical
 * with any list or none — but it decides what the caches see: in plain (chunk, slot) order every pose streams its own region of the
 * panorama through the L2s (1M points x 1800 poses: 16.4 GB through the memory side for 41 MB of unique data).  pcl_trim_order ranks the
 * items by the panorama ROW their chunk's centroid projects to (the row does not depend on the yaw), cuts the ranking into bands of about
 * 2.5 MB of texture rows and deals the XCDs contiguous eighths: an XCD's L2 then holds one band of the texture for all the poses
 * (6.6 GB, L2 hit 0.70 -> 0.88).  The list depends on the cloud, the candidate grid and the panorama's size / texel layout, NOT on the query
 * image: build it once per room (two radix sorts of chunks x slots keys) and pass it to every image's launch.  A list built for another
 * cloud size or grid is ignored by the kernel (plain order).  order: pcl_trim_order_bytes(n, K, ngroups) bytes. */
size_t pcl_trim_order_bytes(int64_t n, int K, int ngroups);
size_t pcl_trim_order_workspace_bytes(int64_t n, int K, int ngroups);
int pcl_trim_order(const float *cloud, int64_t n, int pano_format, int H, int W, const float *trans, int K, const float *rot, int R,
                   const void *groups, int ngroups, void *order, void *workspace, size_t workspace_bytes, void *stream);
/* The same for `nimages` query images of ONE room in one launch (the image loop of localize.py:143-223: the candidate grid
 * depends on the cloud only, utils.py:613-616): panos_host = HOST array of nimages device addresses of packed panoramas (one
 * size and texel format; nimages <= 32), loss_tables / count_tables [nimages][K][R].  The cloud is cut into the chunks of the
 * single-image launch, so every image's table has the bits pcl_trim_loss gives it. */
size_t pcl_trim_loss_images_workspace_bytes(int64_t n, int K, int ngroups, int nimages);
int pcl_trim_loss_images(const float *cloud, int64_t n, const void *const *panos_host, int nimages, int pano_format, int H, int W,
                         const float *trans, int K, const float *rot, int R, const void *groups, int ngroups, const void *order,
                         float *loss_tables, float *count_tables, void *workspace, size_t workspace_bytes, void *stream);
/* The same over a cloud of `color_sets` colour sets (pcl_cloud_pack_sets): color_sets == nimages makes image i's blocks read set i (a
 * scalar plane offset), color_sets == 1 is pcl_trim_loss_images.  Same chunks, same work list (it does not depend on the colours), same
 * workspace: image i's table has the bits pcl_trim_loss gives it over pcl_cloud_pack(xyz, rgb_i). */
int pcl_trim_loss_images_sets(const float *cloud, int64_t n, int color_sets, const void *const *panos_host, int nimages, int pano_format, int H,
                              int W, const float *trans, int K, const float *rot, int R, const void *groups, int ngroups, const void *order,
                              float *loss_tables, float *count_tables, void *workspace, size_t workspace_bytes, void *stream);
/* Scatter-min depth mask on the PACKED cloud for B poses (build-defined: the reference imports torch_scatter.scatter_min at
 * utils.py:6 and never calls it; off by default in the loss).  Seen from pose b, every point falls into one cell of an H x W grid by
 * make_pano's pixel formula (utils.py:158-165) — the DEPTH grid, chosen by point density, not the panorama's resolution: a z-buffer
 * hides a point only when an occluder's point shares its cell, and at the panorama's resolution most cells hold one point —
 *   zmin[b][cell] = the smallest ||p|| among the OCCLUDER SAMPLES in the cell: every stride-th point of the packed cloud (1: all)
 *   visible[b][i] = 1 iff ||p_i|| <= (1 + tau) x zmin[b][cell of p_i]                  (every point i, packed point order)
 * Feeds the `visible` argument of pcl_sampling_loss; the GD loop and pcl_sampling_loss_depth look the z-buffer up in the loss kernel
 * instead and never build the byte mask.  workspace: pcl_depth_workspace_bytes(B, H, W).  Contract: after the call the workspace's last
 * round_up(B x H x W x 4, 16) bytes — byte offset pcl_depth_workspace_bytes(B, H, W) - round_up(B x H x W x 4, 16) — hold the B z-buffers
 * [B][H x W] as uint32 words, each the bit pattern of the fp32 value (zmin (1 + tau))^2 of its cell, 0x7f800000 (+inf) for an empty cell.
 * pcl_depth_default (host-only): what is used when a caller does not name them.  Grid: at least 12 occluder samples per cell
 * (depth_w = 2 depth_h, depth_h a multiple of 8, never finer than the H x W panorama); tau = 3.5 pi / depth_h clipped to [0.02, 0.15]
 * (a coarser cell needs a larger tolerance: a surface seen at a grazing angle spans more depth inside it); stride (stride_in = 0): the
 * largest of 1, 2, 4 that keeps depth_h >= 128 — what the mask finds depends on the samples per cell, not on reading every point.
 * Measured against analytic occlusion on a furnished room (tools/depth_recall.py): recall 0.93-0.96, precision 0.93-0.99 for 167k-4M
 * points.  Any output may be NULL. */
int pcl_depth_default(int64_t n, int H, int W, int stride_in, int *depth_h_host, int *depth_w_host, float *tau_host, int *stride_host);
size_t pcl_depth_workspace_bytes(int B, int H, int W);
int pcl_depth_mask(const float *cloud, int64_t n, const float *trans, const float *rot, int B, int H, int W, float tau, int stride,
                   uint8_t *visible, void *workspace, size_t workspace_bytes, void *stream);
/* Residuals, pose information and LM polish under the depth mask (additive to ABI 12; BUILD-DEFINED: the reference has no occlusion test
 * and none of the three).  pcl_point_residuals, pcl_pose_information (objective 0) / pcl_pose_information_l1 (objective 1) and pcl_gn_refine /
 * pcl_gn_refine_l1 for an UNWEIGHTED cloud with one colour set, with the scatter-min depth mask OF THE EVALUATED POSES multiplied into the
 * loss kernel's mask: before the per-point pass the call writes pose records from the pose rows, fills and builds the z-buffers of all B
 * poses on the depth_h x depth_w grid from every stride-th packed point (pcl_depth_mask's z pass), and the pass looks each point's cell up
 * while its texels are in flight: point i counts at pose b iff ||p_i||^2 <= (zmin (1 + tau))^2 of its cell — pcl_sampling_loss_depth's test.
 * pcl_point_residuals_depth: residual[b][i] is pcl_point_residuals' value where the point is visible (the same instructions on the same
 *   inputs), exactly -1 where it is hidden or samples exact black (pcl_robust_weights reads the row unchanged), NaN at a pose that is not
 *   finite.  visible (nullable) is [B][n] bytes in the row's order (order as for pcl_point_residuals): the in-kernel depth decision alone,
 *   1 visible / 0 hidden, which tells "hidden" from "black".
 * pcl_pose_information_depth: the record layout of pcl_pose_information (objective 0; cov nullable) or pcl_pose_information_l1 (objective 1,
 *   delta by that call's rule; cov is not written) with m the product of both masks; the finish kernel is pcl_pose_information's.
 * pcl_gn_refine_depth: pcl_gn_refine's chain (objective 1: pcl_gn_refine_l1's; cov not written) with the objective REBUILT at every trial
 *   pose: evaluation k = 0 .. iters is pose records from the state's trial poses, fill + z pass for all B poses there, the pass gated on
 *   finished poses, the unchanged step kernel — 1 + 5 (iters + 1) launches.  out, info, cov, trace and state as for pcl_gn_refine; the final
 *   record and covariance are those of the returned pose under the mask at that pose.
 * With a tolerance so large that nothing is hidden every output equals the plain call's bit for bit.  pose_stride as for pcl_point_residuals.
 * Workspaces (pose records, z-buffers, partial rows, in that order, nothing read before it is written): the three size queries, 0 for a
 * B, n or grid no call accepts.  No allocation, no host synchronisation.  Eager launches: nothing is claimed about graph capture.
 * PCL_EINVAL, before any launch: what the plain call refuses; depth_h or depth_w below 2 or B z-buffers of 4 GiB or more (pcl_depth_mask's
 * rule); tau < 0 or not finite; stride outside 1..64; an objective that is neither 0 nor 1; with objective 1 a delta outside [2^-20, 4].
 * PCL_EWORKSPACE: workspace_bytes below the query's.
 * Deliberately left out: weights and robust re-weighting under the mask, colour sets, the images and rooms forms, graph capture, any
 * claim about real data. */
size_t pcl_point_residuals_depth_workspace_bytes(int B, int depth_h, int depth_w);
int pcl_point_residuals_depth(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans, const float *rot,
                              int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, const int64_t *order, float *residual,
                              uint8_t *visible, void *workspace, size_t workspace_bytes, void *stream);
size_t pcl_pose_information_depth_workspace_bytes(int64_t n, int B, int depth_h, int depth_w);
int pcl_pose_information_depth(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans, const float *rot,
                               int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, int objective, float delta, float *info,
                               float *cov, void *workspace, size_t workspace_bytes, void *stream);
size_t pcl_gn_depth_workspace_bytes(int64_t n, int B, int depth_h, int depth_w);
int pcl_gn_refine_depth(const float *cloud, int64_t n, const void *pano, int pano_format, int H, int W, const float *trans, const float *rot,
                        int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, int objective, float delta,
                        const pcl_gn_hyper *hyper_host, int iters, void *state, float *out, float *info, float *cov, float *trace, void *workspace,
                        size_t workspace_bytes, void *stream);
/* ---- colour preprocessing of the query panorama (color_utils.py; called at localize.py:173-179, :395-409) ----
 *
 * pcl_color_template_build: the point colours rgb [n][3] sorted per channel, tmpl [3][n] — once per cloud.
 * pcl_color_match (color_utils.py:146-234): histogram matching of the non-black pixels of img [H][W][3] (levels k/255,
 *   as decoded from an image file) to the point colours, per channel, with sin(latitude) pixel weights, the reference's
 *   wrapped interpolation (period 360) and its rank-indexed lookup.  out [H][W][3]; black pixels are copied.
 *   *not_exact (device int32, nullable) = 1 when some non-black pixel channel is not exactly k/255: the output is then
 *   not the reference's (its lookup is by distinct float value) and the Python layer raises.
 *   DEVIATION: without a non-black pixel, or when every non-black pixel lies in row 0 (weight sin(0) = 0: any image of one row),
 *   the reference raises an IndexError (0 / 0 quantiles); here out = img and nothing is flagged.
 * pcl_color_mod (color_utils.py:7-65): joint luma equalisation.  Panorama (non-black pixels) and point colours go to
 *   8-bit YCrCb (OpenCV's fixed-point cvtColor, restated), the two Y histograms with num_bins levels are added, Y becomes
 *   the joint cumulative distribution at its level, back to RGB.  out_img [H][W][3], out_rgb [n][3].
 * workspace for both: pcl_color_workspace_bytes(). */
size_t pcl_color_template_bytes(int64_t n);
size_t pcl_color_template_workspace_bytes(int64_t n);
int pcl_color_template_build(const float *rgb, int64_t n, float *tmpl, void *workspace, size_t workspace_bytes, void *stream);
size_t pcl_color_workspace_bytes(void);
int pcl_color_match(const float *img_hwc, int H, int W, const float *tmpl, int64_t n, float *out, int32_t *not_exact,
                    void *workspace, size_t workspace_bytes, void *stream);
int pcl_color_mod(const float *img_hwc, int H, int W, const float *rgb, int64_t n, int num_bins, float *out_img,
                  float *out_rgb, void *workspace, size_t workspace_bytes, void *stream);
/* color_utils.py:68-118 histogram (unbatched form): colours img [npix][3] (scaled by 255 first if max(img) <= 1), pixels
 * with mask[p] != 0, c0 x c1 x c2 bins of size ceil(255 / c); hist [c0*c1*c2] float, index r + c0 g + c0 c1 b;
 * normalize: hist / (sum + eps) (eps 0 = unbatched form, 1e-6 = the batched form's).  color_utils.py:122-144
 * histogram_intersection: out[i] = sum_k min(a[i][k], b[i][k]). */
size_t pcl_histogram_workspace_bytes(int c0, int c1, int c2);
int pcl_histogram(const float *img, const uint8_t *mask, int64_t npix, int c0, int c1, int c2, int normalize, float eps,
                  float *hist, void *workspace, size_t workspace_bytes, void *stream);
/* color_utils.py:103-117, the batched form: img [batch][npix][3], mask [batch][npix] -> hist [batch][c0*c1*c2].  The reference asks
 * `max(img) <= 1` of the whole batch (:88), so ONE maximum over all images decides the scale of every image (a black image in a
 * 0..255 batch is not scaled); each image is then counted as pcl_histogram counts it. */
size_t pcl_histogram_batch_workspace_bytes(int batch, int c0, int c1, int c2);
int pcl_histogram_batch(const float *img, const uint8_t *mask, int batch, int64_t npix, int c0, int c1, int c2, int normalize, float eps,
                        float *hist, void *workspace, size_t workspace_bytes, void *stream);
int pcl_histogram_intersection(const float *a, const float *b, int batch, int nbins, float *out, void *stream);
/* p = R (x - t) for one pose: xyz [n][3] -> out [n][3] (feeds make_pano / scatter-min; localize.py:266-267). */
int pcl_transform_cloud(const float *xyz, int64_t n, const float *trans, const float *rot, float *out, void *stream);

/* ---- dataset text clouds (host side, no GPU involved) ----
 * data_utils.py:16-43 read_stanford / :138-163 read_omniscenes parse "x y z r g b" lines with
 * pandas.read_table(header=None, delim_whitespace=True).values.  pcl_cloud_txt_rows: number of non-blank lines
 * (< 0: -errno).  pcl_cloud_txt_read: rows x cols doubles, row-major, parsed by `nthreads` threads (0 = all cores)
 * from an mmap of the file; returns 0, -errno, PCL_EINVAL (bad arguments / row count mismatch) or -(1000 + line) for
 * the first malformed line (1-based). */
int64_t pcl_cloud_txt_rows(const char *path);
int64_t pcl_cloud_txt_read(const char *path, int64_t rows, int cols, double *out, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* PICCOLO_HIP_H */
