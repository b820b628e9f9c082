// pcl_depth_info.hip — per-point residuals, the pose information matrix and the Levenberg-Marquardt polish UNDER THE DEPTH MASK (additive to
// ABI 12; BUILD-DEFINED).  The depth mask of a pose is a function of that pose: whoever evaluates a pose under it
// builds the pose's z-buffer first.  Every evaluation here is therefore
//   pcl_depth_pose_rows_kernel   PclPoseRecs from trans + b * pose_stride / rot + b * pose_stride (pcl_write_pose_rec: the R of the pass)
//   pcl_launch_zbuffers          fill + z pass of all B poses at those records (pcl_depth.hip; the one pcl_depth_mask runs)
//   the depth form of the pass   pcl_point_pass_at<.., DEPTH = true>: the look-ups in flight with the texels, the loss kernel's own test
// and then what the plain entry point does with the pass's output (nothing / the finish kernel / the step kernel, which are launched
// through their own translation units: pcl_info_launch_finish, pcl_gn_launch_step).  Unweighted, one colour set: a weighted cloud is
// refused under the mask everywhere upstream.  The kernels are instances of the texts the plain kernels are instances of; they live in a
// translation unit of their own so that no existing code object function changes.  No atomics (the z pass has its own), no scratch, no
// LDS beyond the pass's reduction rows, no allocation, no host synchronisation.
// Host side: the three entry points share one setup (depth_call_setup: every check that is not an entry point's own, the workspace layout)
// and one z-buffer step (depth_zbuffers_at); the two that take an objective take it as (objective, delta).  The polish is pcl_gn_chain
// with a pass callback that builds the z-buffers first: a launch that fails there or in the step ends the chain at once.
// Outside the loss-kernel hash: the four files it covers are included, never edited.
#include <math.h>

#include "pcl_gn_device.h"
#include "pcl_info_device.h"
#include "pcl_point_pass.h"

// Pose records from strided pose rows: pose_stride 3 reads plain [B][3] arrays, 16 pcl_gd_winner's rows, sizeof(PclGnState) / 4 the
// trial poses of a polish state in place.  (pcl_depth_pose_setup_kernel of pcl_depth.hip reads [B][3] only and stays as it is.)
__global__ void __launch_bounds__(PCL_BLOCK) pcl_depth_pose_rows_kernel(const float* __restrict__ trans, const float* __restrict__ rot, int pose_stride,
                                                                       int B, PclPoseRec* __restrict__ recs)
{
    const int b = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (b >= B) return;
    const float* __restrict__ tp = trans + (int64_t)b * pose_stride;
    const float* __restrict__ rp = rot + (int64_t)b * pose_stride;
    const float p[6] = {tp[0], tp[1], tp[2], rp[0], rp[1], rp[2]};
    pcl_write_pose_rec(&recs[b], p);
}

struct PclResDepthArgs {
    PclPassArgs pass;
    PclPassDepth dz;
    const int64_t* order;    // ORDERED: packed slot -> the caller's point index
    float* residual;         // [B][n]
    uint8_t* visible;        // nullable, [B][n], the row's order: the depth decision alone
};

// Row b of the residuals under pose b's z-buffer: a visible point's value is pcl_point_residuals' (the same instructions on the same
// inputs), a hidden one's acc is (0, 0) and reads -1 like a black sample; `visible` tells the two apart.
template <int FMT, bool ORDERED>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_point_residuals_depth_kernel(PclResDepthArgs a)
{
    const int64_t n = a.pass.n;
    const unsigned b = blockIdx.x % (unsigned)a.pass.B;
    float* __restrict__ row = a.residual + (int64_t)b * n;
    uint8_t* __restrict__ vrow = a.visible ? a.visible + (int64_t)b * n : nullptr;      // (wave-uniform)
    pcl_point_pass<FMT, false, false, true>(
        a.pass, a.pass.pano, 1, 0,
        [&](int i0, int, bool valid0, bool valid1, const f2* acc, bool pose_ok, bool vis0, bool vis1) {
            const float r0 = pcl_res_value(acc[0].x, acc[1].x, pose_ok), r1 = pcl_res_value(acc[0].y, acc[1].y, pose_ok);
            if (valid0) {
                int64_t o = i0;
                if constexpr (ORDERED) o = a.order[i0];
                if ((uint64_t)o < (uint64_t)n) {
                    row[o] = r0;
                    if (vrow) vrow[o] = vis0 ? 1 : 0;
                }
            }
            if (valid1) {
                int64_t o = i0 + 1;
                if constexpr (ORDERED) o = a.order[i0 + 1];
                if ((uint64_t)o < (uint64_t)n) {
                    row[o] = r1;
                    if (vrow) vrow[o] = vis1 ? 1 : 0;
                }
            }
        },
        &a.dz);
}

// The depth instances of pcl_pose_info_kernel and pcl_gn_pass_kernel: the same blocks, chunking, partial rows and reduction order
template <int FMT, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pose_info_depth_kernel(PclInfoArgs a, PclPassDepth dz, PclInfoL1 l1)
{
    pcl_info_pass_at<FMT, false, false, L1, true>(a, PclPassCloud{a.pass.cloud, a.pass.n, a.pass.stride, a.pass.steps_base, a.pass.steps_rem},
                                                  blockIdx.x % (unsigned)a.pass.B, blockIdx.x / (unsigned)a.pass.B, a.pass.pano, 1, 0, 1, 0, a.partials,
                                                  blockIdx.x, l1.inv_delta, l1.half_delta, &dz);
}

template <int FMT, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_depth_kernel(PclInfoArgs a, PclPassDepth dz, PclInfoL1 l1, const PclGnState* __restrict__ state)
{
    if (state[blockIdx.x % (unsigned)a.pass.B].frozen) return;      // (a scalar load: the address depends on the block alone)
    pcl_info_pass_at<FMT, false, false, L1, true>(a, PclPassCloud{a.pass.cloud, a.pass.n, a.pass.stride, a.pass.steps_base, a.pass.steps_rem},
                                                  blockIdx.x % (unsigned)a.pass.B, blockIdx.x / (unsigned)a.pass.B, a.pass.pano, 1, 0, 1, 0, a.partials,
                                                  blockIdx.x, l1.inv_delta, l1.half_delta, &dz);
}

// ---- host side

// What every depth entry point checks of its grid, tolerance and stride before anything else happens
static bool depth_args_ok(int64_t n, int B, int depth_h, int depth_w, float tau, int stride, PclDepthGrid* g)
{
    if (!(tau >= 0.f && tau <= 3.402823466e38f) || stride < 1 || stride > 64 || depth_h <= 0 || depth_w <= 0) return false;
    *g = pcl_make_depth_grid(depth_h, depth_w, tau);
    return pcl_depth_grid_check(n, B, *g) == 0;
}

// The workspace of all three families, in the order it is written: pose records, z-buffers, partial rows (rows_bytes 0: none)
struct PclDepthInfoWs {
    PclPoseRec* recs;
    uint32_t* zbuf;
    float* partials;
};
static size_t depth_info_layout(void* base, int B, int depth_h, int depth_w, size_t rows_bytes, PclDepthInfoWs* w)
{
    PclCarve c{(char*)base, 0};
    w->recs = (PclPoseRec*)c.take((size_t)B * sizeof(PclPoseRec));
    w->zbuf = (uint32_t*)c.take(pcl_depth_zbuf_bytes(B, depth_h, depth_w));
    w->partials = rows_bytes ? (float*)c.take(rows_bytes) : nullptr;
    return c.off;
}

static size_t depth_ws_bytes(int64_t n, int B, int depth_h, int depth_w, bool rows)
{
    PclDepthGrid g;
    if (!depth_args_ok(n, B, depth_h, depth_w, 0.f, 1, &g)) return 0;
    const size_t rows_bytes = rows ? pcl_info_workspace_bytes(n, B) : 0;
    if (rows && rows_bytes == 0) return 0;
    PclDepthInfoWs w;
    return depth_info_layout(nullptr, B, depth_h, depth_w, rows_bytes, &w);
}

// What the three entry points have in hand once their arguments are checked, beside the PclPassArgs of their kernel arguments
struct PclDepthCall {
    PclPassDepth dz;         // the grid, and the z-buffers of the workspace
    PclDepthInfoWs w;
    int64_t nchunks;
    int zstride;
    hipStream_t s;
};

// Every check the entry points share, in the order the codes are promised in: the pass's arguments with the form's min_steps, the grid,
// tolerance and stride, the partial rows of (n, B) where the form has them (`rows`) — PCL_EINVAL — and the workspace: PCL_EWORKSPACE
static int depth_call_setup(PclDepthCall* c, PclPassArgs* pass, const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W,
                            const float* trans, const float* rot, int pose_stride, int B, int min_steps, int depth_h, int depth_w, float tau, int stride,
                            bool rows, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = pcl_pass_args(pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, min_steps, &c->nchunks);
    if (rc) return rc;
    if (!depth_args_ok(n, B, depth_h, depth_w, tau, stride, &c->dz.grid)) return PCL_EINVAL;
    const size_t rows_bytes = rows ? pcl_info_workspace_bytes(n, B) : 0;
    if (rows && rows_bytes == 0) return PCL_EINVAL;
    if (workspace_bytes < depth_info_layout(workspace, B, depth_h, depth_w, rows_bytes, &c->w)) return PCL_EWORKSPACE;
    c->dz.zbuf = c->w.zbuf; c->zstride = stride; c->s = (hipStream_t)stream;
    return 0;
}

// records and z-buffers of the B poses (trans + b * pose_stride, rot + b * pose_stride)
static int depth_zbuffers_at(const PclPassArgs& p, const float* trans, const float* rot, int pose_stride, const PclDepthCall& c)
{
    hipLaunchKernelGGL(pcl_depth_pose_rows_kernel, dim3((unsigned)((p.B + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, c.s, trans, rot, pose_stride,
                       p.B, c.w.recs);
    PCL_LAUNCH_CHECK();
    return pcl_launch_zbuffers(p.cloud, p.n, c.w.recs, p.B, c.dz.grid, c.zstride, c.w.zbuf, true, c.s);
}

extern "C" size_t pcl_point_residuals_depth_workspace_bytes(int B, int depth_h, int depth_w) { return depth_ws_bytes(1, B, depth_h, depth_w, false); }

extern "C" int pcl_point_residuals_depth(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                         const float* rot, int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, const int64_t* order,
                                         float* residual, uint8_t* visible, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!residual || !workspace) return PCL_EINVAL;
    PclResDepthArgs a;
    PclDepthCall c;
    int rc = depth_call_setup(&c, &a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, 1, depth_h, depth_w, tau, stride, false, workspace,
                              workspace_bytes, stream);
    if (rc) return rc;
    a.dz = c.dz; a.order = order; a.residual = residual; a.visible = visible;
    rc = depth_zbuffers_at(a.pass, trans, rot, pose_stride, c);
    if (rc) return rc;
    const dim3 grid((unsigned)(c.nchunks * B)), blk(PCL_BLOCK);
    pcl_with_flag(order != nullptr, [&](auto ord) {
        pcl_with_pass_fmt(pano_format, [&](auto fmt) {
            hipLaunchKernelGGL((pcl_point_residuals_depth_kernel<decltype(fmt)::value, decltype(ord)::value>), grid, blk, 0, c.s, a);
        });
    });
    PCL_LAUNCH_CHECK();
    return 0;
}

// objective 0: L2 (l1 unused), 1: Huber-L1 with pcl_info_l1_args' rule on delta
static bool depth_objective_ok(int objective, float delta, PclInfoL1* l1)
{
    l1->inv_delta = 0.f; l1->half_delta = 0.f;
    if (objective == 0) return true;
    return objective == 1 && pcl_info_l1_args(delta, l1);
}

template <class K>
static void with_fmt_l1(int pano_format, bool l1, K&& launch)
{
    pcl_with_flag(l1, [&](auto l) { pcl_with_pass_fmt(pano_format, [&](auto fmt) { launch(fmt, l); }); });
}

extern "C" size_t pcl_pose_information_depth_workspace_bytes(int64_t n, int B, int depth_h, int depth_w)
{
    return depth_ws_bytes(n, B, depth_h, depth_w, true);
}

extern "C" int pcl_pose_information_depth(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                          const float* rot, int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, int objective,
                                          float delta, float* info, float* cov, void* workspace, size_t workspace_bytes, void* stream)
{
    PclInfoL1 l1;
    if (!info || !workspace || !depth_objective_ok(objective, delta, &l1)) return PCL_EINVAL;
    PclInfoArgs a;
    PclDepthCall c;
    int rc = depth_call_setup(&c, &a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, PCL_INFO_MIN_STEPS, depth_h, depth_w, tau, stride,
                              true, workspace, workspace_bytes, stream);
    if (rc) return rc;
    a.weights = nullptr; a.partials = c.w.partials;
    rc = depth_zbuffers_at(a.pass, trans, rot, pose_stride, c);
    if (rc) return rc;
    const dim3 grid((unsigned)(c.nchunks * B)), blk(PCL_BLOCK);
    with_fmt_l1(pano_format, objective == 1, [&](auto fmt, auto l) {
        hipLaunchKernelGGL((pcl_pose_info_depth_kernel<decltype(fmt)::value, decltype(l)::value>), grid, blk, 0, c.s, a, c.dz, l1);
    });
    PCL_LAUNCH_CHECK();
    // (no covariance under the L1 objective, as in pcl_pose_information_l1)
    return pcl_info_launch_finish((const float*)a.partials, (int)c.nchunks, B, trans, rot, pose_stride, info, objective == 1 ? nullptr : cov, c.s);
}

extern "C" size_t pcl_gn_depth_workspace_bytes(int64_t n, int B, int depth_h, int depth_w) { return depth_ws_bytes(n, B, depth_h, depth_w, true); }

// pcl_gn_chain with the objective rebuilt at every trial pose: evaluation k is records from the state's trial poses, fill + z pass of all
// B poses there (fill launch + z pass), the gated depth pass, the unchanged step kernel: 1 + 5 (iters + 1) launches.  A frozen pose's
// z-buffer is still built: the z pass is not gated.
extern "C" int pcl_gn_refine_depth(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans, const float* rot,
                                   int pose_stride, int B, int depth_h, int depth_w, float tau, int stride, int objective, float delta,
                                   const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info, float* cov, float* trace,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    PclInfoL1 l1;
    if (!pcl_gn_entry_ok(hyper_host, iters, state, out, info, workspace) || !depth_objective_ok(objective, delta, &l1)) return PCL_EINVAL;
    PclInfoArgs a;
    PclDepthCall c;
    const int rc = depth_call_setup(&c, &a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, PCL_INFO_MIN_STEPS, depth_h, depth_w, tau,
                                    stride, true, workspace, workspace_bytes, stream);
    if (rc) return rc;
    a.weights = nullptr;
    const dim3 grid((unsigned)(c.nchunks * B)), blk(PCL_BLOCK);
    return pcl_gn_chain(
        a, B, hyper_host, iters, state, trace, c.w.partials, c.s,
        [&](const PclInfoArgs& ak, const PclGnState* st) {
            // (ak.pass.trans / rot / pose_stride: the state's trial poses in place)
            const int zrc = depth_zbuffers_at(ak.pass, ak.pass.trans, ak.pass.rot, ak.pass.pose_stride, c);
            if (zrc) return zrc;
            with_fmt_l1(pano_format, objective == 1, [&](auto fmt, auto l) {
                hipLaunchKernelGGL((pcl_gn_pass_depth_kernel<decltype(fmt)::value, decltype(l)::value>), grid, blk, 0, c.s, ak, c.dz, l1, st);
            });
            return 0;
        },
        [&](const float* partials, PclGnState* st, const pcl_gn_hyper& hp, int k) {
            return pcl_gn_launch_step(partials, (int)c.nchunks, B, st, hp, k, iters, out, info, objective == 1 ? nullptr : cov, trace, c.s);
        });
}
