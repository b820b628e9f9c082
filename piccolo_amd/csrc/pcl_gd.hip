// pcl_gd.hip — second-stage reduction, chain rule to (t, yaw, pitch, roll) and the on-device optimiser epilogue.
//
// Replaces, per GD iteration of the reference: the tail of autograd (omniloc.py:47,254), B x Adam.step and
// B x ReduceLROnPlateau.step(float(loss)) — each a host sync — (omniloc.py:49-50, :256-258), the re-cat of the
// parameters (omniloc.py:260-263) and the clamp to the quantile box (omniloc.py:52-58, :265-269).
// One 256-thread block per candidate pose (four waves gather the partial sums, wave 0 runs the optimiser update in the
// same precision mix as the reference: fp32 tensors, python-double scalars).
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "pcl_gd_device.h"
#include "pcl_gd_state.h"
#include "pcl_host.h"
#include "pcl_timer.h"

#define PCL_GD_MAX_IMAGES 64     // panorama addresses per pcl_gd_set_pano_groups launch (they travel as kernel arguments)

// ---------------------------------------------------------------- stateless loss: pose setup + finish

__global__ void pcl_pose_setup_kernel(const float* __restrict__ trans, const float* __restrict__ rot, int B, PclPoseRec* recs)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float p[6] = {trans[3 * b], trans[3 * b + 1], trans[3 * b + 2], rot[3 * b], rot[3 * b + 1], rot[3 * b + 2]};
    pcl_write_pose_rec(&recs[b], p);
}

// one block per pose group: second-stage sums (the same fixed order as the GD epilogue), then thread g finishes pose g
template <int G>
__global__ void __launch_bounds__(PCL_GD_THREADS) pcl_finish_kernel(const float* __restrict__ partials, int nchunks, int B,
                                                                    const PclPoseRec* __restrict__ recs,
                                                                    const float* __restrict__ rot, int with_grad,
                                                                    float* __restrict__ result)
{
    __shared__ double rows_sh[(PCL_GD_THREADS / 16) * 2 * G][4];
    __shared__ double sums_sh[G][PCL_NACC];
    pcl_reduce_group<G>(partials, nchunks, blockIdx.x, threadIdx.x, rows_sh, sums_sh);
    if (threadIdx.x < G) {
        const int b = blockIdx.x * G + threadIdx.x;
        double s[PCL_NACC];
        for (int q = 0; q < PCL_NACC; q++) s[q] = sums_sh[threadIdx.x][q];
        float loss, g[6] = {0, 0, 0, 0, 0, 0};
        if (with_grad) {
            double sy, cy, sp, cp;
            sincos((double)rot[3 * b], &sy, &cy);
            sincos((double)rot[3 * b + 1], &sp, &cp);
            pcl_chain_rule(s, recs[b].R, sy, cy, sp, cp, loss, g);
        } else loss = (float)s[0] / (float)s[1];
        float* r = result + (int64_t)b * PCL_RESULT_STRIDE;
        r[0] = loss; r[1] = (float)s[1];
        for (int k = 0; k < 6; k++) r[2 + k] = g[k];
    }
}

// the grid and occluder stride a depth-masked call uses: the caller's, or pcl_depth_default's for 0 x 0 / stride 0 (a given grid
// without a stride: every point builds the z-buffer)
static int gd_depth_grid(int64_t n, int H, int W, int depth_h, int depth_w, float tau, int stride_in, PclDepthGrid* g, int* stride)
{
    if (depth_h < 0 || depth_w < 0 || (depth_h == 0) != (depth_w == 0) || !(tau >= 0.f) || stride_in < 0 || stride_in > 64) return PCL_EINVAL;
    int st = stride_in;
    if (depth_h == 0) {
        int rc = pcl_depth_default(n, H, W, stride_in, &depth_h, &depth_w, nullptr, &st);
        if (rc) return rc;
    } else if (st == 0) st = 1;
    if (stride) *stride = st;
    // (each side below 2^24: the in-kernel lookup addresses its cell with a 24-bit multiply, pcl_sample_device.h)
    if (depth_h < 2 || depth_w < 2 || depth_h >= (1 << 24) || depth_w >= (1 << 24) || (int64_t)depth_h * depth_w > ((int64_t)1 << 28)) return PCL_EINVAL;
    *g = pcl_make_depth_grid(depth_h, depth_w, tau);
    return 0;
}

// (every workspace layout below is one function over a PclCarve, pcl_host.h: the size query runs it without a base)
// stateless loss: pose records and partials back to back; with a depth grid the poses' z-buffers from the next 256-byte boundary on
struct GdLossWs { PclPoseRec* recs; float* partials; uint32_t* zbuf; };
static size_t gd_loss_layout(void* base, int64_t n, int B, const PclDepthGrid* grid, GdLossWs* w)
{
    PclCarve c{(char*)base, 0};
    w->recs = (PclPoseRec*)c.raw((size_t)B * sizeof(PclPoseRec));
    w->partials = (float*)c.raw(pcl_partials_bytes(n, B));
    w->zbuf = nullptr;
    if (grid) {
        c.off = pcl_align256(c.off);
        w->zbuf = (uint32_t*)c.raw(pcl_depth_zbuf_bytes(B, grid->Hd, grid->Wd));
    }
    return c.off;
}

extern "C" size_t pcl_loss_workspace_bytes(int64_t n, int B)
{
    GdLossWs w;
    return n <= 0 || B <= 0 ? 0 : gd_loss_layout(nullptr, n, B, nullptr, &w);
}

// (the default grid follows the occluder stride — 1M points: 144 x 288 at the default stride 2, 200 x 400 at stride 1 — so the size query
//  takes the stride the call will be given: ADVICE r05, a 0 x 0 grid with an explicit stride overflowed a workspace sized without it)
extern "C" size_t pcl_loss_depth_workspace_bytes(int64_t n, int B, int H, int W, int depth_h, int depth_w, int depth_stride)
{
    PclDepthGrid g;
    GdLossWs w;
    if (n <= 0 || B <= 0 || gd_depth_grid(n, H, W, depth_h, depth_w, 0.f, depth_stride, &g, nullptr)) return 0;
    return gd_loss_layout(nullptr, n, B, &g, &w);
}

// pose records, (with a grid: fill + z pass, pcl_depth.hip,) loss launch, finish; the workspace is sized from the grid the caller RESOLVED
// `weights` (nullable): the cloud's weight plane (pcl_sampling_loss_weighted; neither `visible` nor a grid with it)
static int gd_stateless_loss(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans, const float* rot, int B,
                             int with_grad, const uint8_t* visible, const PclDepthGrid* grid, int zstride, float* result, void* workspace,
                             size_t workspace_bytes, hipStream_t s, const float* weights = nullptr)
{
    GdLossWs w;
    if (workspace_bytes < gd_loss_layout(workspace, n, B, grid, &w)) return PCL_EWORKSPACE;
    hipLaunchKernelGGL(pcl_pose_setup_kernel, dim3((B + 255) / 256), dim3(256), 0, s, trans, rot, B, w.recs);
    PCL_LAUNCH_CHECK();
    PclDepthLook look;
    if (grid) {
        look.zbuf = w.zbuf; look.grid = *grid; look.zclear = nullptr; look.zclear_vec4 = 0;
        int rc = pcl_launch_zbuffers(cloud, n, w.recs, B, *grid, zstride, w.zbuf, true, s);
        if (rc) return rc;
    }
    int rc = pcl_launch_loss(cloud, n, pano, pano_format, H, W, w.recs, B, with_grad != 0, visible, w.partials, s, 0, nullptr, grid ? &look : nullptr, 1,
                             weights);
    if (rc) return rc;
    const int nch = pcl_plan_nchunks(n, B);
    pcl_with_G<4>(pcl_plan_G(n, B), [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL(pcl_finish_kernel<G>, dim3(B / G), dim3(PCL_GD_THREADS), 0, s, w.partials, nch, B, w.recs, rot, with_grad, result);
    });
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_sampling_loss(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                 const float* rot, int B, int with_grad, const uint8_t* visible, float* result,
                                 void* workspace, size_t workspace_bytes, void* stream)
{
    if (!cloud || !pano || !trans || !rot || !result || !workspace || n <= 0 || B <= 0 || H <= 0 || W <= 0) return PCL_EINVAL;
    if (n > PCL_MAX_POINTS) return PCL_EINVAL;               // (before anything is enqueued)
    return gd_stateless_loss(cloud, n, pano, pano_format, H, W, trans, rot, B, with_grad, visible, nullptr, 1, result, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

// pcl_sampling_loss over a cloud with per-point weights: loss = sum w m ||d|| / sum w m, the count column sum w m (include/piccolo_hip.h)
extern "C" int pcl_sampling_loss_weighted(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W,
                                          const float* trans, const float* rot, int B, int with_grad, float* result, void* workspace,
                                          size_t workspace_bytes, void* stream)
{
    if (!cloud || !weights || !pano || !trans || !rot || !result || !workspace || n <= 0 || B <= 0 || H <= 0 || W <= 0) return PCL_EINVAL;
    if (!pcl_weighted_plan_ok(n, B)) return PCL_EINVAL;                  // (before anything is enqueued)
    return gd_stateless_loss(cloud, n, pano, pano_format, H, W, trans, rot, B, with_grad, nullptr, nullptr, 1, result, workspace, workspace_bytes,
                             (hipStream_t)stream, weights);
}

// pcl_sampling_loss with the scatter-min depth mask of the SAME poses multiplied into the mask: the loss launch looks every point's
// cell up.  Four launches, no byte mask.
extern "C" int pcl_sampling_loss_depth(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                       const float* rot, int B, int with_grad, int depth_h, int depth_w, float tau, int depth_stride, float* result,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    if (!cloud || !pano || !trans || !rot || !result || !workspace || n <= 0 || B <= 0 || H <= 0 || W <= 0) return PCL_EINVAL;
    if (n > PCL_MAX_POINTS) return PCL_EINVAL;
    PclDepthGrid grid;
    int zstride = 1;
    int rc = gd_depth_grid(n, H, W, depth_h, depth_w, tau, depth_stride, &grid, &zstride);
    if (rc) return rc;
    return gd_stateless_loss(cloud, n, pano, pano_format, H, W, trans, rot, B, with_grad, nullptr, &grid, zstride, result, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

// ---------------------------------------------------------------- GD: state init, epilogue, run, result

// (the state blob's layout — gd_copy_bytes, gd_poses, gd_recs — is pcl_gd_state.h's)

// per_image > 0 (pcl_gd_hyper.color_sets > 1): candidate b reads colour set b / per_image
__global__ void pcl_gd_init_kernel(PclGdPose* st, PclPoseRec* recs, PclPoseRec* recs_shadow, const float* __restrict__ trans,
                                   const float* __restrict__ rot, int B, double lr, int per_image)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    PclGdPose g;
    g.lr = lr;
    g.best = __builtin_inf();   // ReduceLROnPlateau: mode_worse = +inf
    for (int k = 0; k < 3; k++) { g.leaf[k] = trans[3 * b + k]; g.leaf[3 + k] = rot[3 * b + k]; }
    for (int k = 0; k < 6; k++) { g.fwd[k] = g.leaf[k]; g.m[k] = 0.f; g.v[k] = 0.f; }
    g.last_loss = 0.f; g.num_bad = 0; g.step = 0; g.pad = 0;
    g.beta1_pow = 1.0; g.beta2_pow = 1.0;
    recs[b].pano_lo = 0u; recs[b].pano_hi = 0u; recs[b].cset = per_image > 0 ? (uint32_t)(b / per_image) : 0u; recs[b].pad = 0.f;
    pcl_write_pose_rec_fast(&recs[b], g.fwd, g.sc);
    recs_shadow[b] = recs[b];
    st[b] = g;
}

template <int G>
__global__ void __launch_bounds__(PCL_GD_THREADS) pcl_gd_epilogue_kernel(const float* __restrict__ partials, int nchunks,
                                                                         const PclGdPose* st_in, const PclPoseRec* recs_in,
                                                                         PclGdPose* st_out, PclPoseRec* recs_out,
                                                                         const float* __restrict__ box, double factor,
                                                                         int patience, int mode, float* loss_out)
{
    __shared__ double rows_sh[(PCL_GD_THREADS / 16) * 2 * G][4];
    __shared__ double sums_sh[G][PCL_NACC];
    pcl_gd_finish_group<G, false>(partials, nchunks, blockIdx.x, threadIdx.x, st_in, recs_in, st_out, recs_out, true, box, factor, patience, mode,
                                  loss_out, rows_sh, sums_sh, nullptr);
}

// the epilogue's update path driven by a GIVEN loss and gradient per candidate (one block per candidate, G = 1)
__global__ void __launch_bounds__(PCL_GD_THREADS) pcl_gd_forced_kernel(const float* __restrict__ zero_partials, PclGdPose* st, PclPoseRec* recs,
                                                                       const float* __restrict__ box, double factor, int patience, int mode,
                                                                       const float* __restrict__ forced_loss, const float* __restrict__ forced_grad)
{
    __shared__ double rows_sh[(PCL_GD_THREADS / 16) * 2][4];
    __shared__ double sums_sh[1][PCL_NACC];
    pcl_gd_finish_group<1, false, true>(zero_partials, 1, blockIdx.x, threadIdx.x, st, recs, st, recs, true, box, factor, patience, mode, nullptr,
                                        rows_sh, sums_sh, nullptr, forced_loss, forced_grad);
}

__global__ void pcl_gd_result_kernel(const PclGdPose* __restrict__ st, int B, float* __restrict__ result)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* r = result + (int64_t)b * PCL_GD_RESULT_STRIDE;
    for (int k = 0; k < 6; k++) { r[k] = st[b].fwd[k]; r[6 + k] = st[b].leaf[k]; }
    r[12] = st[b].last_loss;
    r[13] = (float)st[b].lr;
    r[14] = (float)st[b].num_bad;
    r[15] = (float)st[b].best;
}

extern "C" size_t pcl_gd_state_bytes(int B) { return B > 0 ? 2 * gd_copy_bytes(B) : 0; }

// colour sets of a run: 1 (the cloud's one set, or 0 / 1 in the hyper-parameters) or hyper->color_sets; -1 when that does not split B
// or is combined with the depth mask (pcl_gd_run's own loss pass has no colour-set instance with the look-up: pcl_gd_run_depth_chain runs those)
static int gd_sets(int B, const pcl_gd_hyper* hyper_host)
{
    if (!hyper_host || hyper_host->color_sets <= 1) return hyper_host && hyper_host->color_sets < 0 ? -1 : 1;
    return B % hyper_host->color_sets || hyper_host->depth_mask ? -1 : hyper_host->color_sets;
}

// single run: two partials buffers (fused iterations read one while they write the other; with colour sets the single-image plan: more
// chunks than the plan of B candidates may have, hence larger partials) and, under the depth mask, two sets of z-buffers: iteration k
// reads set k & 1 and resets the other one for iteration k + 1's z pass (no fill launch between iterations).  Scratch: every pcl_gd_run
// call fills set 0 itself before its first iteration, nothing persists in them.
struct GdRunWs { float* partials[2]; uint32_t* zbuf[2]; };
static size_t gd_run_layout(void* base, int64_t n, int B, int sets, const PclDepthGrid* grid, GdRunWs* w)
{
    PclCarve c{(char*)base, 0};
    for (int k = 0; k < 2; k++) w->partials[k] = (float*)c.take(pcl_partials_bytes(n, B, sets));
    for (int k = 0; k < 2; k++) w->zbuf[k] = grid ? (uint32_t*)c.take(pcl_depth_zbuf_bytes(B, grid->Hd, grid->Wd)) : nullptr;
    return c.off;
}

extern "C" size_t pcl_gd_workspace_bytes(int64_t n, int B, int H, int W, const pcl_gd_hyper* hyper_host)
{
    if (n <= 0 || B <= 0 || !hyper_host) return 0;
    const int sets = gd_sets(B, hyper_host);
    if (sets < 0) return 0;
    PclDepthGrid g;
    GdRunWs w;
    if (hyper_host->depth_mask && gd_depth_grid(n, H, W, hyper_host->depth_h, hyper_host->depth_w, 0.f, hyper_host->depth_stride, &g, nullptr)) return 0;
    return gd_run_layout(nullptr, n, B, sets, hyper_host->depth_mask ? &g : nullptr, &w);
}

extern "C" int pcl_gd_init(void* state, const float* trans, const float* rot, int B, const pcl_gd_hyper* hyper_host, void* stream)
{
    if (!state || !trans || !rot || !hyper_host || B <= 0) return PCL_EINVAL;
    const int sets = gd_sets(B, hyper_host);
    if (sets < 0) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_init_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_poses(state),
                       gd_recs(state, B), gd_recs(state, B, 1), trans, rot, B, hyper_host->lr, sets > 1 ? B / sets : 0);
    PCL_LAUNCH_CHECK();
    return 0;
}

// largest grid that runs ONE launch per iteration: every block resident at once (256 CUs x 4 resident 256-thread blocks);
// pcl_gd_hyper.fuse < 0: never (the two-launch form, bit-identical: what the parity tests compare the fused form with)
static int gd_fuse_limit(const pcl_gd_hyper* hyper_host)
{
    if (hyper_host && hyper_host->fuse < 0) return 0;
    return PCL_KNOB(GD_FUSE_BLOCKS, 1024);                          // (experiments build: read per call)
}

extern "C" int pcl_gd_plan_hyper(int64_t n, int B, const pcl_gd_hyper* hyper_host, int* nchunks_host, int* poses_per_block_host, int* fused_host)
{
    if (n <= 0 || n > PCL_MAX_POINTS || B <= 0) return PCL_EINVAL;
    const int sets = gd_sets(B, hyper_host);
    if (sets < 0) return PCL_EINVAL;
    if (nchunks_host) *nchunks_host = pcl_plan_nchunks(n, B, sets);
    if (poses_per_block_host) *poses_per_block_host = pcl_plan_G(n, B, sets);
    // (the depth-masked loss pass reads a byte mask the fused prologue knows nothing about: pcl_gd_run keeps two launches there)
    const bool depth = hyper_host && hyper_host->depth_mask;
    if (fused_host) *fused_host = (!depth && pcl_plan_nblocks(n, B, sets) <= gd_fuse_limit(hyper_host)) ? 1 : 0;
    return 0;
}

extern "C" int pcl_gd_plan(int64_t n, int B, int* nchunks_host, int* poses_per_block_host, int* fused_host)
{
    return pcl_gd_plan_hyper(n, B, nullptr, nchunks_host, poses_per_block_host, fused_host);
}

// what every run entry point refuses first: a null argument (`what`: its cloud or its rooms), an empty panorama, a negative iteration
// count, an unknown mode
static bool gd_run_args_ok(const void* what, const void* pano, const void* state, const pcl_gd_hyper* hyper_host, const void* workspace, int H, int W,
                           int num_iter)
{
    return what && pano && state && hyper_host && workspace && H > 0 && W > 0 && num_iter >= 0 &&
           (hyper_host->mode == PCL_GD_SEQUENTIAL || hyper_host->mode == PCL_GD_BATCH);
}

// The iteration protocol of every GD chain, once.  Per iteration: before(it) — the z passes of a depth-masked chain —, then the loss
// launch, bracketed by the timer, then the stand-alone epilogue (two-launch form).  Fused form — ONE launch per iteration for launches
// whose blocks are all resident at once (the reference's shipped 167k-point / 6-candidate shape, cfg 1): there an iteration is two
// dependent launches of a few microseconds, and the 5 us the epilogue launch costs are pure dispatch.  The loss launch of iteration
// k + 1 finishes iteration k in the prologue of every block (PclFuseArgs) — no inter-block synchronisation, the kernel boundary is the
// only one: iteration `it` reads copy (it - 1) & 1 of state / pose records / partials and writes copy it & 1, and the last iteration is
// finished by the stand-alone epilogue.  Same arithmetic in the same order: results are bit-identical to the two-launch form.
//   before(it) -> status
//   loss(it, recs, partials_out, fuse) -> status      fuse: null, or the previous iteration to finish (`box`: null where a room table
//                                                      holds every room's own)
//   epilogue(copy_in, partials, loss_out)              reads copy `copy_in` of the state, writes copy 0; loss_out: its row of the history
template <class Before, class Loss, class Epilogue>
static int gd_chain_loop(void* state, int B, bool fused, const float* box, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history,
                         float* const partials2[2], PclTimer* tm, hipStream_t s, Before before, Loss loss, Epilogue epilogue)
{
    auto history = [&](int it) { return loss_history ? loss_history + (int64_t)it * B : nullptr; };
    for (int it = 0; it < num_iter; it++) {
        int rc = before(it);
        if (rc) return rc;
        bool timed;
        hipError_t e = pcl_timer_begin(tm, it, s, &timed);
        if (e != hipSuccess) return (int)e;
        if (fused && it > 0) {
            const int cin = (it - 1) & 1, cout = it & 1;
            PclFuseArgs f;
            f.partials_in = partials2[cin]; f.st_in = gd_poses(state, B, cin); f.recs_in = gd_recs(state, B, cin);
            f.st_out = gd_poses(state, B, cout); f.recs_out = gd_recs(state, B, cout);
            f.box = box; f.factor = hyper_host->factor; f.patience = (int)hyper_host->patience; f.mode = (int)hyper_host->mode;
            f.loss_out = history(it - 1);
            rc = loss(it, f.recs_in, partials2[cout], &f);
        } else {
            rc = loss(it, gd_recs(state, B), partials2[0], nullptr);
        }
        if (rc) return rc;
        if (timed && (e = pcl_timer_end(tm, s)) != hipSuccess) return (int)e;
        if (!fused) {
            epilogue(0, partials2[0], history(it));
            PCL_LAUNCH_CHECK();
        }
    }
    if (fused && num_iter > 0) {
        const int last = num_iter > 1 ? (num_iter - 1) & 1 : 0;    // the copy the last launch wrote (copy 0 when it was the only one)
        epilogue(last, partials2[last], history(num_iter - 1));
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// ---- two half-chains on two streams
// The candidates of a chain are independent until the caller's argmin, so a chain of two launches per iteration may run as TWO chains
// over the pose groups [0, gA) and [gA, ngroups), each under the plan of the whole chain (pcl_launch_loss's group range: the same chunks,
// the same partials rows, the same bits), half A on the caller's stream and half B on a side stream, B half a launch behind A: each
// half's tail, epilogue, kernel boundaries and ramp then run under the other half's bulk.  No launch waits for another inside the loop.
// The side stream (non-blocking: a caller on the legacy default stream is not serialised with it) and the three events exist once per
// device, created on first use by a caller whose stream is not capturing, under a relaxed capture mode so that a capture another
// thread has open is not invalidated.  `mu` is held for the whole enqueue of a split chain: two host threads take turns, so an event
// recorded by one is never re-recorded by the other between its record and its wait.
#define PCL_GD_MAX_DEVICES 64
struct GdSide {
    std::mutex mu;
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, stagger = nullptr, join = nullptr;
};
static GdSide gd_sides[PCL_GD_MAX_DEVICES];

// the current device's side stream with `mu` LOCKED, or null (then nothing is locked): the caller's stream is capturing or cannot be
// asked, the device is out of range, or the stream and events cannot be created — the chain then runs on the caller's stream alone
static GdSide* gd_side_acquire(hipStream_t s)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusActive;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PCL_GD_MAX_DEVICES) return nullptr;
    GdSide* sd = &gd_sides[dev];
    sd->mu.lock();
    if (!sd->ready) {
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        bool ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
        if (ok) {
            ok = hipStreamCreateWithFlags(&sd->stream, hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&sd->fork, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&sd->stagger, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&sd->join, hipEventDisableTiming) == hipSuccess;
            (void)hipThreadExchangeStreamCaptureMode(&mode);
        }
        if (!ok) {
            (void)hipGetLastError();
            if (sd->fork) (void)hipEventDestroy(sd->fork);
            if (sd->stagger) (void)hipEventDestroy(sd->stagger);
            if (sd->join) (void)hipEventDestroy(sd->join);
            if (sd->stream) (void)hipStreamDestroy(sd->stream);
            sd->stream = nullptr; sd->fork = sd->stagger = sd->join = nullptr;
            sd->mu.unlock();
            return nullptr;
        }
        sd->ready = true;
    }
    return sd;
}

// smallest half (in loss blocks) that is split by default.  Measured, eager chains of 100 iterations, one stream against two:
// halves of 528 blocks -5.6 %, 656 +8.8 %, 672 +0.0 %, 896 +16.5 %, 1312 +25.9 %, 1344 +21.1 %, 2048 +4 to +12 % — below about two thirds of
// a residency (256 CUs x 4 resident 256-thread blocks = 1024) the two halves of an iteration fit the GPU together, there is no tail to hide
// and the second stream's launches only cost; 896 is the smallest half measured that clearly gains.
static int gd_split_min_blocks() { return PCL_KNOB(GD_SPLIT_BLOCKS, 896); }

// pcl_gd_run, and with `weights` (the cloud's weight plane) pcl_gd_run_weighted: the same plan, workspace and chain, the weighted loss launch.
// wsets >= 1 (pcl_gd_run_weight_sets): the B candidates are wsets images of B / wsets and the chain runs the single-image plan for all of
// them — its chunks, poses per block and partials — with `weights` null (the plain or colour-set loss launch under that plan) or wsets planes.
static int gd_run(const float* cloud, const float* weights, int wsets, int64_t n, const void* pano, int pano_format, int H, int W, void* state, int B,
                  const float* box, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history, void* workspace, size_t workspace_bytes,
                  void* timer, void* stream)
{
    if (!gd_run_args_ok(cloud, pano, state, hyper_host, workspace, H, W, num_iter) || !box || n <= 0 || n > PCL_MAX_POINTS || B <= 0) return PCL_EINVAL;
    // colour sets: `cloud` holds hyper->color_sets of them (pcl_cloud_pack_sets) and candidate b reads set b / (B / color_sets), as
    // pcl_gd_init wrote into its pose record; the chain runs the single-image plan of B / color_sets candidates (pcl_plan_sets)
    const int sets = gd_sets(B, hyper_host);
    if (sets < 0 || (sets > 1 && pcl_cloud_sets_bytes(n, sets) == 0)) return PCL_EINVAL;
    const int psets = wsets > 0 ? wsets : sets;                  // the images whose single-image plan the chain runs
    hipStream_t s = (hipStream_t)stream;
    const bool depth_on = hyper_host->depth_mask != 0;
    PclDepthLook look;
    look.zbuf = nullptr;
    int zstride = 1;
    if (depth_on) {
        int rcg = gd_depth_grid(n, H, W, hyper_host->depth_h, hyper_host->depth_w, hyper_host->depth_tau, hyper_host->depth_stride, &look.grid, &zstride);
        if (rcg) return rcg;
        look.zclear_vec4 = (int64_t)(pcl_depth_zbuf_bytes(B, look.grid.Hd, look.grid.Wd) / 16);
    }
    GdRunWs w;
    if (workspace_bytes < gd_run_layout(workspace, n, B, psets, depth_on ? &look.grid : nullptr, &w)) return PCL_EWORKSPACE;
    static const int pingpong_env = PCL_KNOB(ZPINGPONG, 1);      // 0: a fill launch per iteration (A/B)
    const int nchunks = pcl_plan_nchunks(n, B, psets);
    // odd iterations walk every XCD's chunks backwards: the first blocks of a launch then read the chunks the previous launch
    // finished with, still in that XCD's L2 (PCL_FLIP=0 turns it off; +0.3 % at cfg 2 in two A/B alternations on one box —
    // the first round of a launch stays 6 us slower than the later ones, so cold L2 is not what makes it slow)
    static const int flip_env = PCL_KNOB(FLIP, 1);
    // several panoramas in the launch AND a cloud small enough to live in every XCD's L2 next to a texture (6 MB: the reference's
    // shipped 167k points): the XCDs split the pose groups — the images — instead of the chunks (pcl_launch_loss).  Large clouds keep
    // the chunk mapping: measured at 1M points, 8 images per launch +0.3 % (3 523 -> 3 533), 5 images per launch (the driver's shape:
    // 10 groups per XCD straddling the images, every XCD walking the whole 24 MB cloud) -1.5 % (3 533 -> 3 479).
    const int xcd_bit = hyper_host->images > 1 && n * 24 <= ((int64_t)6 << 20) ? 2 : 0;
    // (the depth-masked loss pass looks a mask up that the fused prologue knows nothing about: two launches there; pcl_gd_hyper.fuse < 0:
    //  never fused — the form the parity tests compare the fused one with)
    const bool fused = !depth_on && pcl_plan_nblocks(n, B, psets) <= gd_fuse_limit(hyper_host);
    const int G = pcl_plan_G(n, B, psets);
    const int ngroups = B / G;
    // two half-chains (above): pose groups [0, gA) on the caller's stream, [gA, ngroups) on the side stream.  pcl_gd_hyper.fuse -2: never;
    // -3: whenever there are two groups; else when the smaller half has gd_split_min_blocks() loss blocks.  A capturing caller keeps the one-stream chain.
    const int gA = ngroups / 2;
    GdSide* side = nullptr;
    if (!fused && !depth_on && num_iter > 0 && ngroups >= 2 && hyper_host->fuse != -2 &&
        (hyper_host->fuse == -3 || (int64_t)gA * nchunks >= gd_split_min_blocks()))
        side = gd_side_acquire(s);
    if (side) {
        // fork: the side stream starts behind everything the caller has enqueued
        hipError_t e = hipEventRecord(side->fork, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(side->stream, side->fork, 0);
        if (e != hipSuccess) { side->mu.unlock(); return (int)e; }
    }
    auto loss_range = [&](int it, const PclPoseRec* recs, float* partials, hipStream_t st, int g0, int g1) {
        return pcl_launch_loss(cloud, n, pano, pano_format, H, W, recs, B, true, nullptr, partials, st, (flip_env ? (it & 1) : 0) | xcd_bit, nullptr, nullptr,
                               sets, weights, wsets, g0, g1);
    };
    auto epilogue_range = [&](const float* partials, float* loss_out, hipStream_t st, int g0, int g1) {
        pcl_with_G<4>(G, [&](auto g) {
            constexpr int GG = decltype(g)::value;
            const int64_t p0 = (int64_t)g0 * GG;
            hipLaunchKernelGGL(pcl_gd_epilogue_kernel<GG>, dim3(g1 - g0), dim3(PCL_GD_THREADS), 0, st, partials + (int64_t)g0 * nchunks * GG * PCL_NACC, nchunks,
                               gd_poses(state, B, 0) + p0, gd_recs(state, B, 0) + p0, gd_poses(state, B, 0) + p0, gd_recs(state, B, 0) + p0, box,
                               hyper_host->factor, (int)hyper_host->patience, (int)hyper_host->mode, loss_out ? loss_out + p0 : nullptr);
        });
    };
    int rc = gd_chain_loop(
        state, B, fused, box, hyper_host, num_iter, loss_history, w.partials, (PclTimer*)timer, s,
        [&](int it) {
            if (!depth_on) return 0;
            // the scatter-min z-buffers of the poses this iteration evaluates: z pass into set it & 1 (filled by this call before its
            // first iteration, reset by the previous iteration's loss launch afterwards); the loss launch looks them up
            const int set = pingpong_env ? (it & 1) : 0;
            look.zbuf = w.zbuf[set];
            look.zclear = pingpong_env ? w.zbuf[set ^ 1] : nullptr;
            return pcl_launch_zbuffers(cloud, n, gd_recs(state, B), B, look.grid, zstride, w.zbuf[set], it == 0 || !pingpong_env, s);
        },
        [&](int it, const PclPoseRec* recs, float* partials, const PclFuseArgs* fuse) {
            if (!side)
                return pcl_launch_loss(cloud, n, pano, pano_format, H, W, recs, B, true, nullptr, partials, s, (flip_env ? (it & 1) : 0) | xcd_bit, fuse,
                                       depth_on ? &look : nullptr, sets, weights, wsets);
            // half A (what the timer brackets), then half B.  The stagger: A's first launch goes out as two, and B's first launch waits for
            // the first of them — B runs half a launch behind A from there on
            int rcl;
            if (it == 0 && gA >= 2) {
                if ((rcl = loss_range(it, recs, partials, s, 0, gA / 2))) return rcl;
                hipError_t e = hipEventRecord(side->stagger, s);
                if (e == hipSuccess) e = hipStreamWaitEvent(side->stream, side->stagger, 0);
                if (e != hipSuccess) return (int)e;
                if ((rcl = loss_range(it, recs, partials, s, gA / 2, gA))) return rcl;
            } else if ((rcl = loss_range(it, recs, partials, s, 0, gA))) return rcl;
            return loss_range(it, recs, partials, side->stream, gA, ngroups);
        },
        [&](int copy_in, const float* partials, float* loss_out) {
            if (side) {
                epilogue_range(partials, loss_out, s, 0, gA);
                epilogue_range(partials, loss_out, side->stream, gA, ngroups);
                return;
            }
            pcl_with_G<4>(G, [&](auto g) {
                constexpr int GG = decltype(g)::value;
                hipLaunchKernelGGL(pcl_gd_epilogue_kernel<GG>, dim3(B / GG), dim3(PCL_GD_THREADS), 0, s, partials, nchunks, gd_poses(state, B, copy_in),
                                   gd_recs(state, B, copy_in), gd_poses(state, B, 0), gd_recs(state, B, 0), box, hyper_host->factor,
                                   (int)hyper_host->patience, (int)hyper_host->mode, loss_out);
            });
        });
    if (side) {
        // join (after an error too: the side stream's work stays ordered before whatever the caller enqueues next)
        hipError_t e = hipEventRecord(side->join, side->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, side->join, 0);
        side->mu.unlock();
        if (!rc && e != hipSuccess) rc = (int)e;
    }
    return rc;
}

extern "C" int pcl_gd_run(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, void* state, int B,
                          const float* box, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history,
                          void* workspace, size_t workspace_bytes, void* timer, void* stream)
{
    return gd_run(cloud, nullptr, 0, n, pano, pano_format, H, W, state, B, box, hyper_host, num_iter, loss_history, workspace, workspace_bytes, timer, stream);
}

// pcl_gd_run over a cloud with per-point weights: one more caller of the chain loop, with the weighted loss launch (fused or not by the
// same rule); neither the depth mask nor colour sets
extern "C" int pcl_gd_run_weighted(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, void* state,
                                   int B, const float* box, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history, void* workspace,
                                   size_t workspace_bytes, void* timer, void* stream)
{
    if (!weights || !hyper_host || hyper_host->depth_mask || hyper_host->color_sets > 1) return PCL_EINVAL;
    if (!pcl_weighted_plan_ok(n, B)) return PCL_EINVAL;                  // (before the state is touched)
    return gd_run(cloud, weights, 0, n, pano, pano_format, H, W, state, B, box, hyper_host, num_iter, loss_history, workspace, workspace_bytes, timer, stream);
}

// ---------------------------------------------------------------- one weight plane per query image (robust chains over several images)

// what the weight-set entry points refuse: a set count that does not split B, colour sets that are not the weight sets, the depth mask, a
// cloud of that many colour sets past the addressing limit, a plan whose poses per block do not divide an image's candidates or have no
// weighted instance
static bool gd_weight_sets_ok(int64_t n, int B, int nsets, const pcl_gd_hyper* hyper_host)
{
    if (!hyper_host || n <= 0 || n > PCL_MAX_POINTS || B <= 0 || nsets < 1 || B % nsets) return false;
    if (hyper_host->depth_mask || hyper_host->color_sets < 0 || (hyper_host->color_sets > 1 && hyper_host->color_sets != nsets)) return false;
    if (hyper_host->color_sets > 1 && pcl_cloud_sets_bytes(n, nsets) == 0) return false;
    const int G = pcl_plan_G(n, B, nsets);
    return G <= 2 && (B / nsets) % G == 0;
}

extern "C" size_t pcl_gd_weight_sets_workspace_bytes(int64_t n, int B, int nsets, const pcl_gd_hyper* hyper_host)
{
    GdRunWs w;
    return gd_weight_sets_ok(n, B, nsets, hyper_host) ? gd_run_layout(nullptr, n, B, nsets, nullptr, &w) : 0;
}

extern "C" int pcl_gd_plan_weight_sets(int64_t n, int B, int nsets, const pcl_gd_hyper* hyper_host, int* nchunks_host, int* poses_per_block_host,
                                       int* fused_host)
{
    if (!gd_weight_sets_ok(n, B, nsets, hyper_host)) return PCL_EINVAL;
    if (nchunks_host) *nchunks_host = pcl_plan_nchunks(n, B, nsets);
    if (poses_per_block_host) *poses_per_block_host = pcl_plan_G(n, B, nsets);
    if (fused_host) *fused_host = pcl_plan_nblocks(n, B, nsets) <= gd_fuse_limit(hyper_host) ? 1 : 0;
    return 0;
}

// pcl_gd_init for a chain of nsets images: candidate b's pose records (both copies) name image b / (B / nsets) in `cset`, with shared
// colours too — what the weight-set instances of the loss kernel select their plane by (the instances without colour sets never read it)
extern "C" int pcl_gd_init_weight_sets(void* state, const float* trans, const float* rot, int B, int nsets, const pcl_gd_hyper* hyper_host, void* stream)
{
    if (!state || !trans || !rot || !hyper_host || B <= 0 || nsets < 1 || B % nsets) return PCL_EINVAL;
    if (hyper_host->depth_mask || hyper_host->color_sets < 0 || (hyper_host->color_sets > 1 && hyper_host->color_sets != nsets)) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_init_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_poses(state), gd_recs(state, B),
                       gd_recs(state, B, 1), trans, rot, B, hyper_host->lr, B / nsets);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_gd_run_weight_sets(const float* cloud, const float* weights, int nsets, int64_t n, const void* pano, int pano_format, int H, int W,
                                      void* state, int B, const float* box, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history,
                                      void* workspace, size_t workspace_bytes, void* timer, void* stream)
{
    if (!gd_weight_sets_ok(n, B, nsets, hyper_host)) return PCL_EINVAL;                  // (before the state is touched)
    return gd_run(cloud, weights, nsets, n, pano, pano_format, H, W, state, B, box, hyper_host, num_iter, loss_history, workspace, workspace_bytes, timer,
                  stream);
}

// ---------------------------------------------------------------- room search: several clouds in one chain

// The stand-alone epilogue of a multi-room chain: block = pose group of the whole launch; room r owns groups [r ngroups, (r + 1) ngroups)
// and its group is finished from the room's own partials region over the room's own nchunks and clamped to the room's own box — with
// pointers shifted to the room's first candidate, so this is pcl_gd_epilogue_kernel of that room alone.
template <int G>
__global__ void __launch_bounds__(PCL_GD_THREADS) pcl_gd_epilogue_rooms_kernel(const float* __restrict__ partials, const PclRoomTable* __restrict__ rooms,
                                                                               int ngroups, const PclGdPose* st_in, const PclPoseRec* recs_in,
                                                                               PclGdPose* st_out, PclPoseRec* recs_out, double factor, int patience,
                                                                               int mode, float* loss_out)
{
    __shared__ double rows_sh[(PCL_GD_THREADS / 16) * 2 * G][4];
    __shared__ double sums_sh[G][PCL_NACC];
    const int r = (int)blockIdx.x / ngroups, grp = (int)blockIdx.x - r * ngroups;
    const PclRoomRec* rm = rooms->rec + r;
    const int pose0 = pcl_rfl(rm->group0) * G, nchunks = pcl_rfl(rm->nchunks);
    const float* part = partials + (long long)pcl_rfl64((unsigned long long)rm->partials);
    const float* box = (const float*)pcl_rfl64(rm->box);
    pcl_gd_finish_group<G, false>(part, nchunks, grp, threadIdx.x, st_in + pose0, recs_in + pose0, st_out + pose0, recs_out + pose0, true, box, factor,
                                  patience, mode, loss_out ? loss_out + pose0 : nullptr, rows_sh, sums_sh, nullptr);
}

// the room table travels as kernel arguments and is stored with vector stores, one 32-bit word per thread
__global__ void pcl_gd_rooms_table_kernel(PclRoomTable t, PclRoomTable* dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int)(sizeof(PclRoomTable) / 4)) ((int*)dst)[i] = ((const int*)&t)[i];
}

// the host side of a multi-room chain: every room's plan, partials region and block range, the sizes, the checks
struct GdRooms {
    PclRoomTable t;
    int nrooms, per_room, G, ngroups, nblk;   // per_room: candidates of one room (rooms x images chains: of all its images); ngroups likewise
    int sets;                    // colour sets of every room's cloud (rooms x images chains with per-image colours), else 1
    size_t partials_bytes;       // one partials buffer, all rooms (each region 256-byte aligned)
};

// Room r holds nimages * per_image candidates, image by image, and runs the single-image plan pcl_plan(n_r, per_image) for all of them;
// hyper->color_sets is 0 / 1 (the images share the room's colours) or nimages (every room's cloud holds a set per image).
// pcl_gd_run_rooms' chain of one panorama is nimages = 1 (per_image its per_room: the room's own plan, and no colour sets above 1).
static int gd_rooms_setup(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, const pcl_gd_hyper* hyper_host, GdRooms* g)
{
    if (!rooms_host || !hyper_host || nrooms < 1 || nrooms > PCL_GD_MAX_ROOMS || per_image <= 0 || nimages < 1) return PCL_EINVAL;
    if (hyper_host->depth_mask || hyper_host->color_sets < 0) return PCL_EINVAL;
    if (hyper_host->color_sets > 1 && hyper_host->color_sets != nimages) return PCL_EINVAL;
    if ((int64_t)nrooms * per_image * nimages > 0x7fffffff / 2) return PCL_EINVAL;
    const int per_room = per_image * nimages;
    g->sets = hyper_host->color_sets > 1 ? hyper_host->color_sets : 1;
    for (int r = 0; r < nrooms; r++) {
        if (!rooms_host[r].cloud || !rooms_host[r].box || rooms_host[r].n <= 0 || rooms_host[r].n > PCL_MAX_POINTS) return PCL_EINVAL;
        if (g->sets > 1 && pcl_cloud_sets_bytes(rooms_host[r].n, g->sets) == 0) return PCL_EINVAL;
    }
    memset(&g->t, 0, sizeof(g->t));
    g->nrooms = nrooms; g->per_room = per_room;
    int64_t blocks = 0, floats = 0;
    for (int r = 0; r < PCL_GD_MAX_ROOMS; r++) g->t.block0[r] = 0x7fffffff;
    for (int r = 0; r < nrooms; r++) {
        PclRoomRec& e = g->t.rec[r];
        int G, ngroups;
        pcl_plan_room_images(rooms_host[r].n, per_image, nimages, &G, &ngroups, &e.nchunks, &e.seg_len, &e.steps_base, &e.steps_rem);
        g->G = G; g->ngroups = ngroups;              // (pcl_plan's poses per block depend on per_image alone: the same for every room)
        e.cloud = (unsigned long long)rooms_host[r].cloud; e.box = (unsigned long long)rooms_host[r].box;
        e.n = (int)rooms_host[r].n; e.stride = (int)pcl_cloud_stride(rooms_host[r].n);
        e.block0 = (int)blocks; e.group0 = r * ngroups; e.partials = floats;
        g->t.block0[r] = (int)blocks;
        blocks += (int64_t)e.nchunks * ngroups;
        floats += (int64_t)(pcl_align256((size_t)e.nchunks * per_room * PCL_NACC * sizeof(float)) / sizeof(float));
    }
    if (blocks > 0x7fffffff) return PCL_EINVAL;
    g->nblk = (int)blocks;
    g->partials_bytes = (size_t)floats * sizeof(float);
    return 0;
}

// the stand-alone epilogue of a multi-room chain: reads copy `copy_in` of the state, writes copy 0
static void gd_rooms_epilogue(const GdRooms& g, const PclRoomTable* table, void* state, int copy_in, const float* partials, const pcl_gd_hyper* hyper_host,
                              float* lo, hipStream_t s)
{
    const int B = g.nrooms * g.per_room;
    pcl_with_G<2>(g.G, [&](auto gg) {
        hipLaunchKernelGGL(pcl_gd_epilogue_rooms_kernel<decltype(gg)::value>, dim3(g.nrooms * g.ngroups), dim3(PCL_GD_THREADS), 0, s, partials, table,
                           g.ngroups, gd_poses(state, B, copy_in), gd_recs(state, B, copy_in), gd_poses(state, B, 0), gd_recs(state, B, 0),
                           hyper_host->factor, (int)hyper_host->patience, (int)hyper_host->mode, lo);
    });
}

// multi-room chain: the room table, then two partials buffers (fused iterations read one while they write the other).  Depth-masked
// chain (`depth`): room table, depth table, ONE partials buffer — such a chain never fuses, so partials[1] stays null and gd_chain_loop
// never reads it —, two z-buffer sets of zset_bytes each.
struct GdRoomsWs { PclRoomTable* table; PclDepthTable* dtab; float* partials[2]; uint32_t* zset[2]; };
static size_t gd_rooms_layout(void* base, const GdRooms& g, bool depth, size_t zset_bytes, GdRoomsWs* w)
{
    PclCarve c{(char*)base, 0};
    w->table = (PclRoomTable*)c.take(sizeof(PclRoomTable));
    w->dtab = depth ? (PclDepthTable*)c.take(sizeof(PclDepthTable)) : nullptr;
    w->partials[0] = (float*)c.take(g.partials_bytes);
    w->partials[1] = depth ? nullptr : (float*)c.take(g.partials_bytes);
    for (int k = 0; k < 2; k++) w->zset[k] = depth ? (uint32_t*)c.take(zset_bytes) : nullptr;
    return c.off;
}

// the iteration loop of a multi-room chain whose plan `g` holds: table launch, then per iteration the rooms loss launch (+ the rooms
// epilogue in the two-launch form); flip and timer as in pcl_gd_run, and the XCDs always split the chunks
static int gd_rooms_chain(const GdRooms& g, const void* pano, int pano_format, int H, int W, void* state, const pcl_gd_hyper* hyper_host, int num_iter,
                          float* loss_history, void* workspace, PclTimer* tm, hipStream_t s)
{
    const int B = g.nrooms * g.per_room;
    GdRoomsWs w;
    gd_rooms_layout(workspace, g, false, 0, &w);
    const int words = (int)(sizeof(PclRoomTable) / 4);
    hipLaunchKernelGGL(pcl_gd_rooms_table_kernel, dim3((words + 255) / 256), dim3(256), 0, s, g.t, w.table);
    PCL_LAUNCH_CHECK();
    static const int flip_env = PCL_KNOB(FLIP, 1);
    return gd_chain_loop(
        state, B, g.nblk <= gd_fuse_limit(hyper_host), nullptr, hyper_host, num_iter, loss_history, w.partials, tm, s, [](int) { return 0; },
        [&](int it, const PclPoseRec* recs, float* partials, const PclFuseArgs* fuse) {
            return pcl_launch_loss_rooms(w.table, pano, pano_format, H, W, recs, B, g.G, g.ngroups, g.nblk, partials, s, flip_env ? (it & 1) : 0, fuse,
                                         g.sets);
        },
        [&](int copy_in, const float* partials, float* lo) { gd_rooms_epilogue(g, w.table, state, copy_in, partials, hyper_host, lo, s); });
}

// the one-image entry points: the rooms x images functions with nimages = 1 (which then admit neither colour sets above 1 nor, as ever,
// the depth mask)
extern "C" size_t pcl_gd_rooms_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int per_room, const pcl_gd_hyper* hyper_host)
{
    return pcl_gd_rooms_images_workspace_bytes(rooms_host, nrooms, 1, per_room, hyper_host);
}

extern "C" int pcl_gd_plan_rooms(const pcl_gd_room* rooms_host, int nrooms, int per_room, const pcl_gd_hyper* hyper_host, int* nchunks_host,
                                 int* poses_per_block_host, int* fused_host)
{
    return pcl_gd_plan_rooms_images(rooms_host, nrooms, 1, per_room, hyper_host, nchunks_host, poses_per_block_host, fused_host);
}

extern "C" int pcl_gd_run_rooms(const pcl_gd_room* rooms_host, int nrooms, const void* pano, int pano_format, int H, int W, void* state, int per_room,
                                const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history, void* workspace, size_t workspace_bytes,
                                void* timer, void* stream)
{
    return pcl_gd_run_rooms_images(rooms_host, nrooms, 1, pano, pano_format, H, W, state, per_room, hyper_host, num_iter, loss_history, workspace,
                                   workspace_bytes, timer, stream);
}

// ---------------------------------------------------------------- room search: several panoramas x several rooms in one chain

extern "C" size_t pcl_gd_rooms_images_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, const pcl_gd_hyper* hyper_host)
{
    GdRooms g;
    GdRoomsWs w;
    if (gd_rooms_setup(rooms_host, nrooms, nimages, per_image, hyper_host, &g)) return 0;
    return gd_rooms_layout(nullptr, g, false, 0, &w);
}

extern "C" int pcl_gd_plan_rooms_images(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, const pcl_gd_hyper* hyper_host,
                                        int* nchunks_host, int* poses_per_block_host, int* fused_host)
{
    GdRooms g;
    const int rc = gd_rooms_setup(rooms_host, nrooms, nimages, per_image, hyper_host, &g);
    if (rc) return rc;
    if (nchunks_host)
        for (int r = 0; r < nrooms; r++) nchunks_host[r] = g.t.rec[r].nchunks;
    if (poses_per_block_host) *poses_per_block_host = g.G;
    if (fused_host) *fused_host = g.nblk <= gd_fuse_limit(hyper_host) ? 1 : 0;
    return 0;
}

// candidate b of a rooms x images state belongs to image (b / per_image) % nimages: its colour set
__global__ void pcl_gd_set_csets_kernel(PclPoseRec* recs, PclPoseRec* recs_shadow, int B, int per_image, int nimages)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t c = (uint32_t)((b / per_image) % nimages);
    recs[b].cset = c; recs_shadow[b].cset = c;
}

extern "C" int pcl_gd_init_rooms_images(void* state, const float* trans, const float* rot, int nrooms, int nimages, int per_image,
                                        const pcl_gd_hyper* hyper_host, void* stream)
{
    if (!state || !trans || !rot || !hyper_host || nrooms < 1 || nrooms > PCL_GD_MAX_ROOMS || nimages < 1 || per_image < 1) return PCL_EINVAL;
    if ((int64_t)nrooms * nimages * per_image > 0x7fffffff / 2) return PCL_EINVAL;
    if (hyper_host->color_sets < 0 || (hyper_host->color_sets > 1 && hyper_host->color_sets != nimages)) return PCL_EINVAL;
    const int B = nrooms * nimages * per_image;
    hipLaunchKernelGGL(pcl_gd_init_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_poses(state), gd_recs(state, B),
                       gd_recs(state, B, 1), trans, rot, B, hyper_host->lr, 0);
    PCL_LAUNCH_CHECK();
    if (hyper_host->color_sets > 1) {
        hipLaunchKernelGGL(pcl_gd_set_csets_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_recs(state, B), gd_recs(state, B, 1), B,
                           per_image, nimages);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// pcl_gd_run for several rooms and panoramas: the same iteration loop, fused and two-launch forms, with the rooms instances of the loss
// kernel and the rooms epilogue
extern "C" int pcl_gd_run_rooms_images(const pcl_gd_room* rooms_host, int nrooms, int nimages, const void* pano, int pano_format, int H, int W,
                                       void* state, int per_image, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history, void* workspace,
                                       size_t workspace_bytes, void* timer, void* stream)
{
    if (!gd_run_args_ok(rooms_host, pano, state, hyper_host, workspace, H, W, num_iter)) return PCL_EINVAL;
    GdRooms g;
    GdRoomsWs w;
    const int rc = gd_rooms_setup(rooms_host, nrooms, nimages, per_image, hyper_host, &g);
    if (rc) return rc;
    if (workspace_bytes < gd_rooms_layout(nullptr, g, false, 0, &w)) return PCL_EWORKSPACE;
    // one room and one image: pcl_gd_run itself (the same plan and arithmetic — and no room look-up in front of every block: 1.2 us per
    // iteration at the shipped shape, tools/room_bench.py).  Its workspace, two partials buffers of the same plan, fits in this one.
    if (nrooms == 1 && nimages == 1) {
        pcl_gd_hyper h = *hyper_host;
        h.images = 0; h.color_sets = 0;
        return pcl_gd_run(rooms_host[0].cloud, rooms_host[0].n, pano, pano_format, H, W, state, per_image, rooms_host[0].box, &h, num_iter, loss_history,
                          workspace, workspace_bytes, timer, stream);
    }
    return gd_rooms_chain(g, pano, pano_format, H, W, state, hyper_host, num_iter, loss_history, workspace, (PclTimer*)timer, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the depth mask inside a shared chain: colour sets, rooms, rooms x images

// both tables of a depth-masked chain in one launch (kernel arguments, vector stores; 3.2 KB of the 4 KB argument block)
__global__ void pcl_gd_depth_tables_kernel(PclRoomTable t, PclDepthTable d, PclRoomTable* dst_t, PclDepthTable* dst_d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int NT = (int)(sizeof(PclRoomTable) / 4), ND = (int)(sizeof(PclDepthTable) / 4);
    if (i < NT) ((int*)dst_t)[i] = ((const int*)&t)[i];
    else if (i < NT + ND) ((int*)dst_d)[i - NT] = ((const int*)&d)[i - NT];
}

// the host side of a depth-masked chain: the rooms plan of the same hyper-parameters without the mask, plus every room's own grid,
// tolerance and occluder stride (gd_depth_grid: what a pcl_gd_run of that room resolves) and its region of a z-buffer set
struct GdDepthChain {
    GdRooms g;
    PclDepthTable d;
    int zstride[PCL_GD_MAX_ROOMS];
    size_t zset_bytes;           // one z-buffer set: every room's per_room z-buffers, each region a whole number of 16-byte words
};

static int gd_depth_chain_setup(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, int H, int W, const pcl_gd_hyper* hyper_host,
                                GdDepthChain* c)
{
    if (!rooms_host || !hyper_host || H <= 0 || W <= 0 || !hyper_host->depth_mask) return PCL_EINVAL;
    pcl_gd_hyper h = *hyper_host;
    h.depth_mask = 0;
    int rc = gd_rooms_setup(rooms_host, nrooms, nimages, per_image, &h, &c->g);
    if (rc) return rc;
    memset(&c->d, 0, sizeof(c->d));
    size_t bytes = 0;
    for (int r = 0; r < nrooms; r++) {
        PclRoomDepth& e = c->d.rec[r];
        rc = gd_depth_grid(rooms_host[r].n, H, W, hyper_host->depth_h, hyper_host->depth_w, hyper_host->depth_tau, hyper_host->depth_stride, &e.grid,
                           &c->zstride[r]);
        if (rc) return rc;
        // (one 32-bit buffer descriptor per room in the loss kernel: pcl_depth_check's limit)
        if ((int64_t)c->g.per_room * e.grid.Hd * e.grid.Wd * 4 >= ((int64_t)1 << 32)) return PCL_EINVAL;
        e.stride = c->zstride[r];
        e.zoff = (long long)(bytes / sizeof(uint32_t));
        bytes += pcl_depth_zbuf_bytes(c->g.per_room, e.grid.Hd, e.grid.Wd);
    }
    c->zset_bytes = bytes;
    return 0;
}

// one room and one image: pcl_gd_run itself (hyper without colour sets and without the image hint)
static pcl_gd_hyper gd_depth_single_hyper(const pcl_gd_hyper* hyper_host)
{
    pcl_gd_hyper h = *hyper_host;
    h.color_sets = 0; h.images = 0;
    return h;
}

extern "C" size_t pcl_gd_depth_chain_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, int H, int W,
                                                     const pcl_gd_hyper* hyper_host)
{
    GdDepthChain c;
    GdRoomsWs w;
    if (gd_depth_chain_setup(rooms_host, nrooms, nimages, per_image, H, W, hyper_host, &c)) return 0;
    size_t bytes = gd_rooms_layout(nullptr, c.g, true, c.zset_bytes, &w);
    if (nrooms == 1 && nimages == 1) {           // (forwarded to pcl_gd_run: its workspace has to fit as well)
        const pcl_gd_hyper h = gd_depth_single_hyper(hyper_host);
        const size_t single = pcl_gd_workspace_bytes(rooms_host[0].n, per_image, H, W, &h);
        if (single > bytes) bytes = single;
    }
    return bytes;
}

extern "C" int pcl_gd_plan_depth_chain(const pcl_gd_room* rooms_host, int nrooms, int nimages, int per_image, int H, int W,
                                       const pcl_gd_hyper* hyper_host, int* nchunks_host, int* poses_per_block_host, int* depth_h_host,
                                       int* depth_w_host, int* depth_stride_host)
{
    GdDepthChain c;
    const int rc = gd_depth_chain_setup(rooms_host, nrooms, nimages, per_image, H, W, hyper_host, &c);
    if (rc) return rc;
    for (int r = 0; r < nrooms; r++) {
        if (nchunks_host) nchunks_host[r] = c.g.t.rec[r].nchunks;
        if (depth_h_host) depth_h_host[r] = c.d.rec[r].grid.Hd;
        if (depth_w_host) depth_w_host[r] = c.d.rec[r].grid.Wd;
        if (depth_stride_host) depth_stride_host[r] = c.zstride[r];
    }
    if (poses_per_block_host) *poses_per_block_host = c.g.G;
    return 0;
}

// Per iteration: every room's z pass (the existing launch, on the room's cloud, pose range and region of set it & 1), ONE loss launch over
// all rooms that looks the masks up and resets the other set, ONE rooms epilogue.  Timer and flip as in pcl_gd_run.
extern "C" int pcl_gd_run_depth_chain(const pcl_gd_room* rooms_host, int nrooms, int nimages, const void* pano, int pano_format, int H, int W,
                                      void* state, int per_image, const pcl_gd_hyper* hyper_host, int num_iter, float* loss_history,
                                      void* workspace, size_t workspace_bytes, void* timer, void* stream)
{
    if (!gd_run_args_ok(rooms_host, pano, state, hyper_host, workspace, H, W, num_iter)) return PCL_EINVAL;
    GdDepthChain c;
    int rc = gd_depth_chain_setup(rooms_host, nrooms, nimages, per_image, H, W, hyper_host, &c);
    if (rc) return rc;
    if (workspace_bytes < pcl_gd_depth_chain_workspace_bytes(rooms_host, nrooms, nimages, per_image, H, W, hyper_host)) return PCL_EWORKSPACE;
    if (nrooms == 1 && nimages == 1) {
        const pcl_gd_hyper h = gd_depth_single_hyper(hyper_host);
        return pcl_gd_run(rooms_host[0].cloud, rooms_host[0].n, pano, pano_format, H, W, state, per_image, rooms_host[0].box, &h, num_iter, loss_history,
                          workspace, workspace_bytes, timer, stream);
    }
    hipStream_t s = (hipStream_t)stream;
    const GdRooms& g = c.g;
    const int B = nrooms * g.per_room;
    GdRoomsWs w;
    gd_rooms_layout(workspace, g, true, c.zset_bytes, &w);
    const int words = (int)((sizeof(PclRoomTable) + sizeof(PclDepthTable)) / 4);
    hipLaunchKernelGGL(pcl_gd_depth_tables_kernel, dim3((words + 255) / 256), dim3(256), 0, s, g.t, c.d, w.table, w.dtab);
    PCL_LAUNCH_CHECK();
    static const int flip_env = PCL_KNOB(FLIP, 1);
    PclDepthLook look = {};                                   // (every room's grid: the depth table)
    look.zclear_vec4 = (int64_t)(c.zset_bytes / 16);
    return gd_chain_loop(
        state, B, false, nullptr, hyper_host, num_iter, loss_history, w.partials, (PclTimer*)timer, s,
        [&](int it) {
            // (set 0 is filled by this call before its first iteration; afterwards the previous iteration's loss launch reset the set)
            look.zbuf = w.zset[it & 1];
            look.zclear = w.zset[(it & 1) ^ 1];
            for (int r = 0; r < nrooms; r++) {
                const int rcz = pcl_launch_zbuffers(rooms_host[r].cloud, rooms_host[r].n, gd_recs(state, B) + (size_t)r * g.per_room, g.per_room,
                                                    c.d.rec[r].grid, c.zstride[r], w.zset[it & 1] + c.d.rec[r].zoff, it == 0, s);
                if (rcz) return rcz;
            }
            return 0;
        },
        [&](int it, const PclPoseRec* recs, float* partials, const PclFuseArgs* fuse) {
            return pcl_launch_loss_rooms(w.table, pano, pano_format, H, W, recs, B, g.G, g.ngroups, g.nblk, partials, s, flip_env ? (it & 1) : 0, fuse,
                                         g.sets, w.dtab, &look);
        },
        [&](int copy_in, const float* partials, float* lo) { gd_rooms_epilogue(g, w.table, state, copy_in, partials, hyper_host, lo, s); });
}

extern "C" int pcl_gd_step_from_grads(void* state, int B, const float* loss, const float* grad, const float* box, const pcl_gd_hyper* hyper_host,
                                      float* scratch, void* stream)
{
    if (!state || !loss || !grad || !box || !hyper_host || !scratch || B <= 0) return PCL_EINVAL;
    if (hyper_host->mode != PCL_GD_SEQUENTIAL && hyper_host->mode != PCL_GD_BATCH) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(scratch, 0, (size_t)B * PCL_NACC * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_gd_forced_kernel, dim3(B), dim3(PCL_GD_THREADS), 0, s, scratch, gd_poses(state, B, 0), gd_recs(state, B, 0), box,
                       hyper_host->factor, (int)hyper_host->patience, (int)hyper_host->mode, loss, grad);
    PCL_LAUNCH_CHECK();
    return 0;
}

__global__ void pcl_gd_set_panos_kernel(PclPoseRec* recs, PclPoseRec* recs_shadow, const unsigned long long* __restrict__ panos, int B)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    unsigned long long p = panos ? panos[b] : 0ull;
    recs[b].pano_lo = recs_shadow[b].pano_lo = (uint32_t)(p & 0xffffffffull);
    recs[b].pano_hi = recs_shadow[b].pano_hi = (uint32_t)(p >> 32);
}

extern "C" int pcl_gd_set_panos(void* state, const uint64_t* panos, int B, void* stream)
{
    if (!state || B <= 0) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_set_panos_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_recs(state, B),
                       gd_recs(state, B, 1), (const unsigned long long*)panos, B);
    PCL_LAUNCH_CHECK();
    return 0;
}

// The panorama of every candidate from a SHORT host list: image i's address for candidates [i * per_image, (i + 1) * per_image).
// The addresses travel as kernel arguments — no device table, so no host-to-device copy in front of a refinement (a pageable
// H2D copy waits for everything the stream holds: it cost the shipped-shape pipeline its overlap of host and device work).
struct PclPanoList { unsigned long long p[PCL_GD_MAX_IMAGES]; };

__global__ void pcl_gd_set_pano_groups_kernel(PclPoseRec* recs, PclPoseRec* recs_shadow, PclPanoList list, int b0, int count, int per_image)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const unsigned long long p = list.p[j / per_image];
    const int b = b0 + j;
    recs[b].pano_lo = recs_shadow[b].pano_lo = (uint32_t)(p & 0xffffffffull);
    recs[b].pano_hi = recs_shadow[b].pano_hi = (uint32_t)(p >> 32);
}

extern "C" int pcl_gd_set_pano_groups(void* state, const uint64_t* panos_host, int nimages, int per_image, void* stream)
{
    if (!state || !panos_host || nimages <= 0 || per_image <= 0 || (int64_t)nimages * per_image > 0x7fffffff) return PCL_EINVAL;
    const int B = nimages * per_image;
    for (int i0 = 0; i0 < nimages; i0 += PCL_GD_MAX_IMAGES) {
        PclPanoList list;
        const int m = nimages - i0 < PCL_GD_MAX_IMAGES ? nimages - i0 : PCL_GD_MAX_IMAGES;
        for (int i = 0; i < PCL_GD_MAX_IMAGES; i++) list.p[i] = i < m ? (unsigned long long)panos_host[i0 + i] : 0ull;
        const int count = m * per_image;
        hipLaunchKernelGGL(pcl_gd_set_pano_groups_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_recs(state, B),
                           gd_recs(state, B, 1), list, i0 * per_image, count, per_image);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// The end of omniloc_batch (omniloc.py:271-277) for `nimages` images of `per_image` candidates each: the candidate whose LAST
// forward had the smallest loss (torch.argmin: the first of equal minima, and a NaN loss counts as the minimum), its post-step
// translation, R = RZ RY RX of its post-step angles, that loss and the angles: 16 floats per image.  Also hands the leaf
// parameters of all candidates back (the reference optimises views of the caller's tensors in place, omniloc.py:216-219).
// One wave per image: lane-strided scan of the candidates' last losses, a wave argmin with torch.argmin's rules (a NaN beats any
// number, among equals — or among NaNs — the smaller index wins: pcl_gd_better, which pcl_gd_prune ranks by too), lane 0 writes the winner's 16 floats, all lanes the leaf rows.
__global__ void __launch_bounds__(PCL_WAVE) pcl_gd_winner_kernel(const PclGdPose* __restrict__ st, int nimages, int per_image, float* __restrict__ out,
                                                                 float* __restrict__ leaf_trans, float* __restrict__ leaf_rot)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const PclGdPose* s = st + (int64_t)i * per_image;
    float best = 0.f;
    int k = PCL_GD_NO_CANDIDATE;                               // (none yet)
    for (int b = lane; b < per_image; b += PCL_WAVE) {
        const float l = s[b].last_loss;
        if (pcl_gd_better(l, b, best, k)) { best = l; k = b; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float lo = __shfl_xor(best, o, 64);
        const int ko = __shfl_xor(k, o, 64);
        if (pcl_gd_better(lo, ko, best, k)) { best = lo; k = ko; }
    }
    if (lane == 0) {
        float* o = out + (int64_t)i * 16;
        float R[9];
        pcl_rot_from_ypr(s[k].fwd[3], s[k].fwd[4], s[k].fwd[5], R);
        for (int q = 0; q < 3; q++) { o[q] = s[k].fwd[q]; o[13 + q] = s[k].fwd[3 + q]; }
        for (int q = 0; q < 9; q++) o[3 + q] = R[q];
        o[12] = s[k].last_loss;
    }
    for (int b = lane; b < per_image; b += PCL_WAVE) {
        const int64_t row = ((int64_t)i * per_image + b) * 3;
        for (int q = 0; q < 3; q++) {
            if (leaf_trans) leaf_trans[row + q] = s[b].leaf[q];
            if (leaf_rot) leaf_rot[row + q] = s[b].leaf[3 + q];
        }
    }
}

extern "C" int pcl_gd_winner(const void* state, int nimages, int per_image, float* winners, float* leaf_trans, float* leaf_rot, void* stream)
{
    if (!state || !winners || nimages <= 0 || per_image <= 0) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_winner_kernel, dim3(nimages), dim3(PCL_WAVE), 0, (hipStream_t)stream, (const PclGdPose*)state, nimages,
                       per_image, winners, leaf_trans, leaf_rot);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_gd_result(const void* state, int B, float* result, void* stream)
{
    if (!state || !result || B <= 0) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_result_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const PclGdPose*)state, B, result);
    PCL_LAUNCH_CHECK();
    return 0;
}
