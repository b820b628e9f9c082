// pcl_info.hip — how well the panorama constrains a pose: the Gauss-Newton information matrix of the sampling loss at given poses and
// the covariance that follows from it (additive to ABI 12).  BUILD-DEFINED: the reference returns a pose and a loss and nothing else.
//
//   theta = (t0, t1, t2, yaw, pitch, roll); per point i: mask bit m_i (the loss kernel's), weight w_i (1 without a weight plane),
//   residual l_i = ||c_i - rgb_i||, j_i = d l_i / d theta = C a_i with a_i = [g_i; tau_i], g = d l / d p in the camera frame,
//   tau = p x g, and C the 6 x 6 map of pcl_chain_rule (restated in the finish text, pcl_info_finish_body.h).
//   M = sum w m    S1 = sum w m l    S2 = sum w m l^2    H = sum w m j j^T    b = sum w m l j    sigma^2 = S2 / M    cov = sigma^2 H^-1
//
// pcl_pose_info_kernel is the per-point pass of pcl_point_pass.h, the one pcl_point_residuals_kernel is (256 threads, a lane carries the two
// ADJACENT packed slots 2 t, 2 t + 1 of a 512-slot step, R and t in SGPRs, cloud / weights / texels through buffer resources), with the
// weighted gradient instance of pcl_sample2 under UNIT weight and fresh accumulators — so that after a step acc[0], acc[1], acc[2..7]
// are that pair of points' own l, mask, g, tau: the very numbers the loss kernel would have added (a masked or invalid point has l = 0
// and a = 0 through its 1/||d|| = 0).  What this kernel adds is what becomes of a pair.  The weight enters ONCE, here: a lane forms w a_k
// (exact for w = 1) and adds (w a_k) a_l, (w a_k) l, (w l) l, w l, w m with one fma each into 30 packed-fp32 accumulators, every one of
// them named at compile time (fully unrolled loops: a runtime-indexed register array would live in scratch).  Squaring a weighted
// gradient would give w^2.
// The block then adds the two packed halves, the 64 lanes of a wave (DPP) and the four waves (LDS) in a fixed order and stores one
// partial row of 32 floats per (chunk, pose).  No atomics, no scratch; the grid is chunks x poses with the pose varying fastest.
// pcl_pose_info_finish_kernel: one block per pose adds the chunks' rows in double in a fixed order, forms H = C A C^T and b = C v in
// double, factorises (Cholesky), inverts, and rounds every output once to fp32.  Same inputs, same bits.
// The L1 instances of the pass (pcl_pose_information_l1, pcl_pose_information_images_l1) put the IRLS weight
// phi = min(1 / l, 1 / delta) on the 21 + 6 moment sums and sum w m rho(l) where S2 goes; M and S1 stay plain and the finish is unchanged.
// Host side: one body per form, a template over the objective (pcl_info_single<L1>, pcl_info_images<L1>; the rooms form has L2 alone and is
// its own entry point).  A body holds the form's checks and the one place that picks the pass instance; the finish kernel is launched
// from pcl_info_launch_finish and nowhere else.  An extern "C" function checks what is its own and calls its instance of the body.
#include <math.h>

#include "pcl_info_device.h"
#include "pcl_point_pass.h"
#include "pcl_sample_device.h"

// (the pass is pcl_info_pass of pcl_info_device.h, which pcl_gn.hip runs as well, gated)
template <int FMT, bool WT>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_kernel(PclInfoArgs a)
{
    pcl_info_pass<FMT, WT>(a, a.pass.pano, 1, 0, 1, 0, blockIdx.x);
}

// Pose b against panorama b (pcl_pose_information_images): block chunk * a.pass.B + b of a launch of a.pass.B images evaluates pose b
// against im.panos.p[b], with CS colour set b + img0 and with per-image planes (im.wsets > 1) weight plane b + img0, into partial row
// chunk * btot + img0 + b.  The same pass: row b has the bits of pcl_pose_info_kernel's row for that pose, panorama, set and plane alone.
template <int FMT, bool WT, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_images_kernel(PclInfoArgs a, PclInfoImages im)
{
    const unsigned b = blockIdx.x % (unsigned)a.pass.B, chunk = blockIdx.x / (unsigned)a.pass.B;      // (from the block index: uniform)
    const unsigned g = b + (unsigned)im.img0;
    pcl_info_pass<FMT, WT, CS>(a, (const void*)im.panos.p[b], im.sets, g, im.wsets, im.wsets > 1 ? (int)g * ((int)a.pass.stride * 4) : 0,
                               chunk * (unsigned)im.btot + g);
}

// The Huber-L1 instances of the two kernels above (pcl_pose_information_l1, pcl_pose_information_images_l1): the same blocks, chunking, partial
// rows and reduction order, with the pass's L1 flag (pcl_info_device.h) and its two wave-uniform floats by value in the kernel arguments.
// They are templates of their own beside their twins, so that every instance that existed before them keeps its name and its text.
template <int FMT, bool WT, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_kernel(PclInfoArgs a, PclInfoL1 l1)
{
    static_assert(L1, "the plain instance is pcl_pose_info_kernel<FMT, WT>");
    pcl_info_pass<FMT, WT, false, L1>(a, a.pass.pano, 1, 0, 1, 0, blockIdx.x, l1.inv_delta, l1.half_delta);
}

template <int FMT, bool WT, bool CS, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_images_kernel(PclInfoArgs a, PclInfoImages im, PclInfoL1 l1)
{
    static_assert(L1, "the plain instance is pcl_pose_info_images_kernel<FMT, WT, CS>");
    const unsigned b = blockIdx.x % (unsigned)a.pass.B, chunk = blockIdx.x / (unsigned)a.pass.B;      // (from the block index: uniform)
    const unsigned g = b + (unsigned)im.img0;
    pcl_info_pass<FMT, WT, CS, L1>(a, (const void*)im.panos.p[b], im.sets, g, im.wsets, im.wsets > 1 ? (int)g * ((int)a.pass.stride * 4) : 0,
                                   chunk * (unsigned)im.btot + g, l1.inv_delta, l1.half_delta);
}

// Pose (r, i) against room r's cloud and panorama i (pcl_pose_information_rooms): the block finds its room, chunk and image from its index
// in the room table of the kernel arguments (pcl_info_room_select) and runs the same pass over that room's cloud into that room's rows.
template <int FMT, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_rooms_kernel(PclInfoArgs a, PclInfoImages im, PclInfoRooms rm)
{
    pcl_info_pass_rooms<FMT, CS>(a, im, pcl_info_room_select(rm, (unsigned)a.pass.B));
}

// The finish: one 256-thread block per pose adds the pose's chunk rows in double in a fixed order, forms H = C A C^T and b = C v, factorises
// and writes the record and the covariance.  Its body is ONE text, pcl_info_finish_body.h, included by both kernels below after a
// prologue that names the pose's rows, pose and outputs (that file says why it is a text, not a function).
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_finish_kernel(const float* __restrict__ partials, int nchunks, int B,
                                                                        const float* __restrict__ trans, const float* __restrict__ rot,
                                                                        int pose_stride, float* __restrict__ info, float* __restrict__ cov)
{
    const int b = blockIdx.x;
#include "pcl_info_finish_body.h"
}

// The finish of pcl_pose_information_rooms: one block per pose (r, i) = blockIdx.x, over room r's own chunk count and region of rows.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_finish_rooms_kernel(const float* __restrict__ partials_all, PclInfoRooms rm, int nimages,
                                                                              const float* __restrict__ trans_all, const float* __restrict__ rot_all,
                                                                              int pose_stride, float* __restrict__ info_all, float* __restrict__ cov_all)
{
    const int pose = blockIdx.x, room = pose / nimages, b = pose - room * nimages, B = nimages, nchunks = rm.rec[room].nchunks;
    const float* __restrict__ partials = partials_all + rm.rec[room].rows;
    const float* __restrict__ trans = trans_all + (int64_t)room * nimages * pose_stride;
    const float* __restrict__ rot = rot_all + (int64_t)room * nimages * pose_stride;
    float* __restrict__ info = info_all + (int64_t)room * nimages * PCL_INFO_REC;
    float* __restrict__ cov = cov_all ? cov_all + (int64_t)room * nimages * 36 : nullptr;
#include "pcl_info_finish_body.h"
}

int pcl_info_launch_finish(const float* partials, int nchunks, int B, const float* trans, const float* rot, int pose_stride, float* info, float* cov,
                           hipStream_t s)
{
    hipLaunchKernelGGL(pcl_pose_info_finish_kernel, dim3((unsigned)B), dim3(PCL_BLOCK), 0, s, partials, nchunks, B, trans, rot, pose_stride, info, cov);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t pcl_pose_information_workspace_bytes(int64_t n, int B) { return pcl_info_workspace_bytes(n, B); }

// The host body of the single form under either objective (pcl_info_device.h: `l1` is read under L1 only): the checks, the one place
// that picks the pass instance, the finish.  Under L1 the record holds H_rho, b_rho, M, S1 (both plain), sum w m rho and F_rho = sum w m rho / M
// in the slots of H, b, M, S1, S2 and sigma^2, and there is no covariance: F_rho H_rho^-1 is not one.
template <bool L1>
static int pcl_info_single(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                           const float* rot, int pose_stride, int B, float* info, float* cov, PclInfoL1 l1, void* workspace, size_t workspace_bytes,
                           void* stream)
{
    if (!info || !workspace) return PCL_EINVAL;
    PclInfoArgs a;
    int64_t nchunks;
    const int rc = pcl_pass_args(&a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, PCL_INFO_MIN_STEPS, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_info_workspace_bytes(n, B)) return PCL_EINVAL;
    a.weights = weights; a.partials = (float*)workspace;
    const dim3 grid((unsigned)(nchunks * B)), blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    pcl_with_flag(weights != nullptr, [&](auto wt) {
        pcl_with_pass_fmt(pano_format, [&](auto fmt) {
            constexpr int FMT = decltype(fmt)::value;
            constexpr bool WT = decltype(wt)::value;
            if constexpr (L1) hipLaunchKernelGGL((pcl_pose_info_kernel<FMT, WT, true>), grid, blk, 0, s, a, l1);
            else hipLaunchKernelGGL((pcl_pose_info_kernel<FMT, WT>), grid, blk, 0, s, a);
        });
    });
    PCL_LAUNCH_CHECK();
    return pcl_info_launch_finish((const float*)a.partials, (int)nchunks, B, trans, rot, pose_stride, info, L1 ? nullptr : cov, s);
}

extern "C" int pcl_pose_information(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W,
                                    const float* trans, const float* rot, int pose_stride, int B, float* info, float* cov, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    return pcl_info_single<false>(cloud, weights, n, pano, pano_format, H, W, trans, rot, pose_stride, B, info, cov, PclInfoL1{}, workspace,
                                  workspace_bytes, stream);
}

extern "C" int pcl_pose_information_l1(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W,
                                       const float* trans, const float* rot, int pose_stride, int B, float* info, void* workspace,
                                       size_t workspace_bytes, float delta, void* stream)
{
    PclInfoL1 l1;
    if (!pcl_info_l1_args(delta, &l1)) return PCL_EINVAL;
    return pcl_info_single<true>(cloud, weights, n, pano, pano_format, H, W, trans, rot, pose_stride, B, info, nullptr, l1, workspace, workspace_bytes,
                                 stream);
}

// The host body of the images form.  Record i = the single form's of pose i against panos_host[i], colour set i and weight plane i: one
// pass launch per PCL_RES_MAX_IMAGES images into the call's [nchunks][nimages] partial rows (the chunking depends on n alone), then the
// finish over all of them.
template <bool L1>
static int pcl_info_images(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets, const uint64_t* panos_host, int nimages,
                           int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride, float* info, float* cov, PclInfoL1 l1,
                           void* workspace, size_t workspace_bytes, void* stream)
{
    if (!info || !workspace) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    int64_t nchunks;
    const int rc = pcl_info_images_args(&a, &im, cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot,
                                        pose_stride, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_info_workspace_bytes(n, nimages)) return PCL_EINVAL;
    a.partials = (float*)workspace;
    const dim3 blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    pcl_info_images_launches(a, im, panos_host, nchunks, [&](const PclInfoArgs& al, const PclInfoImages& il, int, dim3 grid) {
        pcl_with_flag(weights != nullptr, [&](auto wt) {
            pcl_with_flag(color_sets > 1, [&](auto cs) {
                pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                    constexpr int FMT = decltype(fmt)::value;
                    constexpr bool WT = decltype(wt)::value, CS = decltype(cs)::value;
                    if constexpr (L1) hipLaunchKernelGGL((pcl_pose_info_images_kernel<FMT, WT, CS, true>), grid, blk, 0, s, al, il, l1);
                    else hipLaunchKernelGGL((pcl_pose_info_images_kernel<FMT, WT, CS>), grid, blk, 0, s, al, il);
                });
            });
        });
    });
    PCL_LAUNCH_CHECK();
    return pcl_info_launch_finish((const float*)a.partials, (int)nchunks, nimages, trans, rot, pose_stride, info, L1 ? nullptr : cov, s);
}

extern "C" int pcl_pose_information_images(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets,
                                           const uint64_t* panos_host, int nimages, int pano_format, int H, int W, const float* trans, const float* rot,
                                           int pose_stride, float* info, float* cov, void* workspace, size_t workspace_bytes, void* stream)
{
    return pcl_info_images<false>(cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride, info, cov,
                                  PclInfoL1{}, workspace, workspace_bytes, stream);
}

extern "C" int pcl_pose_information_images_l1(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets,
                                              const uint64_t* panos_host, int nimages, int pano_format, int H, int W, const float* trans,
                                              const float* rot, int pose_stride, float* info, void* workspace, size_t workspace_bytes, float delta,
                                              void* stream)
{
    PclInfoL1 l1;
    if (!pcl_info_l1_args(delta, &l1)) return PCL_EINVAL;
    return pcl_info_images<true>(cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride, info, nullptr,
                                 l1, workspace, workspace_bytes, stream);
}

extern "C" size_t pcl_pose_information_rooms_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int nimages)
{
    PclInfoRoomsPlan g;
    return pcl_info_rooms_plan(rooms_host, nrooms, nimages, &g) ? 0 : g.bytes;
}

// Record (r, i) = pcl_pose_information of pose r * nimages + i against room r's cloud, colour set i and panos_host[i]: per
// PCL_RES_MAX_IMAGES images one pass launch over all rooms (each into its own region of rows), then one finish launch over all poses.
extern "C" int pcl_pose_information_rooms(const pcl_gd_room* rooms_host, int nrooms, int color_sets, const uint64_t* panos_host, int nimages,
                                          int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride, float* info, float* cov,
                                          void* workspace, size_t workspace_bytes, void* stream)
{
    if (!info || !workspace) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    PclInfoRoomsPlan g;
    const int rc = pcl_info_rooms_args(&a, &im, &g, rooms_host, nrooms, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride);
    if (rc) return rc;
    if (workspace_bytes < g.bytes) return PCL_EINVAL;
    a.partials = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    pcl_info_rooms_launches(a, im, g, panos_host, [&](const PclInfoArgs& al, const PclInfoImages& il, const PclInfoRooms& tl, int, dim3 grid) {
        pcl_with_flag(color_sets > 1, [&](auto cs) {
            pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                hipLaunchKernelGGL((pcl_pose_info_rooms_kernel<decltype(fmt)::value, decltype(cs)::value>), grid, dim3(PCL_BLOCK), 0, s, al, il, tl);
            });
        });
    });
    PCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pcl_pose_info_finish_rooms_kernel, dim3((unsigned)(nrooms * nimages)), dim3(PCL_BLOCK), 0, s, (const float*)a.partials, g.t, nimages,
                       trans, rot, pose_stride, info, cov);
    PCL_LAUNCH_CHECK();
    return 0;
}
