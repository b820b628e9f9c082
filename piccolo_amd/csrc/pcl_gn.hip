// pcl_gn.hip — a Levenberg-Marquardt polish of poses on the device, built on H and b of pcl_info.hip (additive to ABI 12).  BUILD-DEFINED:
// the reference refines with Adam and has nothing like it.
//
// What is minimised: the MEAN SQUARED residual sigma^2(theta) = sum w m l^2 / sum w m over theta = (t0, t1, t2, yaw, pitch, roll), with the
// Gauss-Newton model H = sum w m j j^T, b = sum w m l j of pcl_info.hip.  This is NOT the sampling loss sum w m l / sum w m that the GD chains
// minimise: the two share their per-point terms, mask and weights and are different objectives.  The mask m is treated as constant
// inside a step (it is re-evaluated at every trial pose).  Nothing is claimed about real data.  The Huber-L1 form at the end of this file
// (pcl_gn_refine_l1, pcl_gn_refine_images_l1) runs the same chain on an objective that tends to the sampling loss itself.
//
// One call enqueues 1 + 2 (iters + 1) launches and nothing else; every decision is taken on the device:
//   pcl_gn_init_kernel        theta_try = theta_acc = the caller's pose, F_acc = +inf, lambda = lam0, counters 0; the trace is zeroed
//   evaluation k = 0 .. iters
//     pcl_gn_pass_kernel      the per-point pass of pcl_pose_info_kernel (pcl_info_pass: same arithmetic, same partial rows) at theta_try, read
//                             from the state; GATED: a block reads its pose's `frozen` word (wave-uniform) and returns before the point loop
//     pcl_gn_step_kernel      one block per pose, frozen poses skipped: the rows in double in pcl_pose_info_finish_kernel's order, H = C A C^T,
//                             b = C v, F = (float)(S2 / M); accept iff the sums are finite, M > 0 and F < F_acc in fp32 (k = 0: iff finite and
//                             M > 0, else status 1); lambda = fmaxf(lambda lam_down, lam_min) on acceptance (not at k = 0), fminf(lambda lam_up,
//                             lam_max) on rejection; then, k < iters, the step on the ACCEPTED sums: (H + lambda diag H) delta = -b by the
//                             finish kernel's Cholesky (a failed pivot: status 2), the whole delta scaled to max |delta_i| = step_cap where it
//                             exceeds it, theta_try = (float)((double)theta_acc + delta); converged (status 3) when max |delta_i| <= tol or
//                             theta_try == theta_acc in all six floats.  A pose that freezes, and every pose at k = iters, writes its outputs:
//                             out, the info record and the covariance at theta_acc, formed from the accepted sums by the device functions
//                             pcl_pose_information forms them with.
// No atomics, no scratch, no host synchronisation, no allocation: capturable (the hyper-parameters are kernel arguments, read from the host
// struct when the call is enqueued).  Poses never interact: pose b of a batch has the bits of its own call.
// pcl_gn_refine_images is the same chain for poses that each have their own panorama, colour set and weight plane (the winners of a chain
// over several query images): pcl_gn_pass_images_kernel in place of the pass, the init and step kernels as they are.
// The chain itself — state as pose source, init launch, the k loop — is pcl_gn_chain of pcl_gn_device.h for every entry point, those of
// pcl_gn_rooms.hip and pcl_depth_info.hip included; a form says how its pass and its step are launched.  Host side here: one body per
// form, a template over the objective (pcl_gn_single<L1>, pcl_gn_images<L1>) with the form's checks and the one place that picks the gated
// pass instance; the step kernel is launched from pcl_gn_launch_step and nowhere else.  An extern "C" function checks what is its own
// and calls its instance of the body.
#include <math.h>

#include "pcl_gn_device.h"
#include "pcl_info_device.h"

__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_init_kernel(PclGnState* __restrict__ state, const float* __restrict__ trans,
                                                               const float* __restrict__ rot, int pose_stride, float lam0, float* __restrict__ trace,
                                                               int B, int iters)
{
    const int b = blockIdx.x;
    if (trace)
        for (int i = threadIdx.x; i < (iters + 1) * PCL_GN_OUT; i += PCL_BLOCK)
            trace[((int64_t)(i / PCL_GN_OUT) * B + b) * PCL_GN_OUT + i % PCL_GN_OUT] = 0.f;
    if (threadIdx.x != 0) return;
    PclGnState& st = state[b];
    for (int i = 0; i < 3; i++) {
        st.acc[i] = st.tri[i] = trans[(int64_t)b * pose_stride + i];
        st.acc[3 + i] = st.tri[3 + i] = rot[(int64_t)b * pose_stride + i];
    }
    for (int i = 0; i < 6; i++) {
        for (int m = 0; m < 6; m++) st.H[i][m] = 0.0;
        st.b[i] = 0.0;
    }
    st.M = 0.0; st.S1 = 0.0; st.S2 = 0.0;
    st.F_acc = __builtin_inff(); st.F_start = __builtin_nanf(""); st.lam = lam0;
    st.accepted = 0; st.rejected = 0; st.evaluations = 0; st.status = 0; st.frozen = 0; st.sums_ok = 0; st.pad = 0;
}

template <int FMT, bool WT>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_kernel(PclInfoArgs a, const PclGnState* __restrict__ state)
{
    if (state[blockIdx.x % (unsigned)a.pass.B].frozen) return;      // (a scalar load: the address depends on the block alone)
    pcl_info_pass<FMT, WT>(a, a.pass.pano, 1, 0, 1, 0, blockIdx.x);
}

// The gated pass of pcl_gn_refine_images: pcl_pose_info_images_kernel's block (pose b against panorama b, colour set and weight plane
// b + img0, partial row chunk * btot + img0 + b) behind the same gate, per pose: `state` is the launch's first image's.
template <int FMT, bool WT, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_images_kernel(PclInfoArgs a, PclInfoImages im, const PclGnState* __restrict__ state)
{
    const unsigned b = blockIdx.x % (unsigned)a.pass.B, chunk = blockIdx.x / (unsigned)a.pass.B;      // (from the block index: uniform)
    if (state[b].frozen) return;
    const unsigned g = b + (unsigned)im.img0;
    pcl_info_pass<FMT, WT, CS>(a, (const void*)im.panos.p[b], im.sets, g, im.wsets, im.wsets > 1 ? (int)g * ((int)a.pass.stride * 4) : 0,
                               chunk * (unsigned)im.btot + g);
}

// The Huber-L1 instances of the two gated passes (pcl_gn_refine_l1, pcl_gn_refine_images_l1): the same gate, blocks and rows, with the pass's L1
// flag and its two floats by value in the kernel arguments.  Templates of their own beside their twins, as in pcl_info.hip.
template <int FMT, bool WT, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_kernel(PclInfoArgs a, const PclGnState* __restrict__ state, PclInfoL1 l1)
{
    static_assert(L1, "the plain instance is pcl_gn_pass_kernel<FMT, WT>");
    if (state[blockIdx.x % (unsigned)a.pass.B].frozen) return;      // (a scalar load: the address depends on the block alone)
    pcl_info_pass<FMT, WT, false, L1>(a, a.pass.pano, 1, 0, 1, 0, blockIdx.x, l1.inv_delta, l1.half_delta);
}

template <int FMT, bool WT, bool CS, bool L1>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_images_kernel(PclInfoArgs a, PclInfoImages im, const PclGnState* __restrict__ state, PclInfoL1 l1)
{
    static_assert(L1, "the plain instance is pcl_gn_pass_images_kernel<FMT, WT, CS>");
    const unsigned b = blockIdx.x % (unsigned)a.pass.B, chunk = blockIdx.x / (unsigned)a.pass.B;      // (from the block index: uniform)
    if (state[b].frozen) return;
    const unsigned g = b + (unsigned)im.img0;
    pcl_info_pass<FMT, WT, CS, L1>(a, (const void*)im.panos.p[b], im.sets, g, im.wsets, im.wsets > 1 ? (int)g * ((int)a.pass.stride * 4) : 0,
                                   chunk * (unsigned)im.btot + g, l1.inv_delta, l1.half_delta);
}

// The step's body is ONE text, pcl_gn_step_body.h, which pcl_gn_step_rooms_kernel of pcl_gn_rooms.hip includes as well, over a room's
// region of rows (that file says why it is a text, not a function).  Here pose b's rows are rows b of [nchunks][B].
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_step_kernel(const float* __restrict__ partials, int nchunks, int B, PclGnState* __restrict__ state,
                                                               pcl_gn_hyper hp, int k, int iters, float* __restrict__ out, float* __restrict__ info,
                                                               float* __restrict__ cov, float* __restrict__ trace)
{
    const int b = blockIdx.x, rowsB = B, row = b;
#include "pcl_gn_step_body.h"
}

int pcl_gn_launch_init(PclGnState* state, const float* trans, const float* rot, int pose_stride, float lam0, float* trace, int B, int iters, hipStream_t s)
{
    hipLaunchKernelGGL(pcl_gn_init_kernel, dim3((unsigned)B), dim3(PCL_BLOCK), 0, s, state, trans, rot, pose_stride, lam0, trace, B, iters);
    PCL_LAUNCH_CHECK();
    return 0;
}

int pcl_gn_launch_step(const float* partials, int nchunks, int B, PclGnState* state, const pcl_gn_hyper& hp, int k, int iters, float* out, float* info,
                       float* cov, float* trace, hipStream_t s)
{
    hipLaunchKernelGGL(pcl_gn_step_kernel, dim3((unsigned)B), dim3(PCL_BLOCK), 0, s, partials, nchunks, B, state, hp, k, iters, out, info, cov, trace);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t pcl_gn_state_bytes(int B)
{
    if (B <= 0) return 0;
    return pcl_align256((size_t)B * sizeof(PclGnState));
}

extern "C" size_t pcl_gn_workspace_bytes(int64_t n, int B) { return pcl_info_workspace_bytes(n, B); }

// The host body of the single form under either objective (pcl_info_device.h: `l1` is read under L1 only): the checks, then the chain
// with the one place that picks the gated pass instance and the step launch.  Under L1 the step kernel gets a null cov.
template <bool L1>
static int pcl_gn_single(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                         const float* rot, int pose_stride, int B, const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info,
                         float* cov, float* trace, PclInfoL1 l1, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pcl_gn_entry_ok(hyper_host, iters, state, out, info, workspace)) return PCL_EINVAL;
    PclInfoArgs a;
    int64_t nchunks;
    const int rc = pcl_pass_args(&a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, PCL_INFO_MIN_STEPS, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_info_workspace_bytes(n, B)) return PCL_EINVAL;
    a.weights = weights;
    const dim3 grid((unsigned)(nchunks * B)), blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    return pcl_gn_chain(
        a, B, hyper_host, iters, state, trace, workspace, s,
        [&](const PclInfoArgs& ak, const PclGnState* st) {
            pcl_with_flag(weights != nullptr, [&](auto wt) {
                pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                    constexpr int FMT = decltype(fmt)::value;
                    constexpr bool WT = decltype(wt)::value;
                    if constexpr (L1) hipLaunchKernelGGL((pcl_gn_pass_kernel<FMT, WT, true>), grid, blk, 0, s, ak, st, l1);
                    else hipLaunchKernelGGL((pcl_gn_pass_kernel<FMT, WT>), grid, blk, 0, s, ak, st);
                });
            });
            return 0;
        },
        [&](const float* partials, PclGnState* st, const pcl_gn_hyper& hp, int k) {
            return pcl_gn_launch_step(partials, (int)nchunks, B, st, hp, k, iters, out, info, L1 ? nullptr : cov, trace, s);
        });
}

// The host body of the images form: pcl_gn_refine for nimages poses, each against ITS OWN panorama, colour set and weight plane, in one
// chain: the init and step launches run over all the images (they are per pose and do not care which image a pose belongs to), the
// gated pass runs once per PCL_RES_MAX_IMAGES images into the call's [nchunks][nimages] partial rows.  1 + (groups + 1) (iters + 1) launches.
template <bool L1>
static int pcl_gn_images(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets, const uint64_t* panos_host, int nimages,
                         int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride, const pcl_gn_hyper* hyper_host, int iters,
                         void* state, float* out, float* info, float* cov, float* trace, PclInfoL1 l1, void* workspace, size_t workspace_bytes,
                         void* stream)
{
    if (!pcl_gn_entry_ok(hyper_host, iters, state, out, info, workspace)) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    int64_t nchunks;
    const int rc = pcl_info_images_args(&a, &im, cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot,
                                        pose_stride, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_info_workspace_bytes(n, nimages)) return PCL_EINVAL;
    const dim3 blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    return pcl_gn_chain(
        a, nimages, hyper_host, iters, state, trace, workspace, s,
        [&](const PclInfoArgs& ak, const PclGnState* st) {
            pcl_info_images_launches(ak, im, panos_host, nchunks, [&](const PclInfoArgs& al, const PclInfoImages& il, int i0, dim3 grid) {
                pcl_with_flag(weights != nullptr, [&](auto wt) {
                    pcl_with_flag(color_sets > 1, [&](auto cs) {
                        pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                            constexpr int FMT = decltype(fmt)::value;
                            constexpr bool WT = decltype(wt)::value, CS = decltype(cs)::value;
                            if constexpr (L1) hipLaunchKernelGGL((pcl_gn_pass_images_kernel<FMT, WT, CS, true>), grid, blk, 0, s, al, il, st + i0, l1);
                            else hipLaunchKernelGGL((pcl_gn_pass_images_kernel<FMT, WT, CS>), grid, blk, 0, s, al, il, st + i0);
                        });
                    });
                });
            });
            return 0;
        },
        [&](const float* partials, PclGnState* st, const pcl_gn_hyper& hp, int k) {
            return pcl_gn_launch_step(partials, (int)nchunks, nimages, st, hp, k, iters, out, info, L1 ? nullptr : cov, trace, s);
        });
}

extern "C" int pcl_gn_refine(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                             const float* rot, int pose_stride, int B, const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info,
                             float* cov, float* trace, void* workspace, size_t workspace_bytes, void* stream)
{
    return pcl_gn_single<false>(cloud, weights, n, pano, pano_format, H, W, trans, rot, pose_stride, B, hyper_host, iters, state, out, info, cov, trace,
                                PclInfoL1{}, workspace, workspace_bytes, stream);
}

extern "C" int pcl_gn_refine_images(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets, const uint64_t* panos_host,
                                    int nimages, int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride,
                                    const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info, float* cov, float* trace,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    return pcl_gn_images<false>(cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride, hyper_host,
                                iters, state, out, info, cov, trace, PclInfoL1{}, workspace, workspace_bytes, stream);
}

// ---- the Huber-L1 form: the same chain on F_rho = sum w m rho(l) / sum w m, rho Huber's function divided by delta,
// with H_rho = sum w m phi j j^T and b_rho = sum w m phi l j, phi = min(1 / l, 1 / delta).  For delta -> 0 F_rho tends to the sampling loss
// and b_rho / M to its gradient; for delta >= max l it is the chain above up to the factor 1 / delta.  Only the pass differs: its L1
// instance puts sum w m rho where S2 goes, and the init, step and finish kernels, the state and pcl_gn_chain run as they are — the step
// accepts on (float)(s[27] / M), which is F_rho, and solves on the accepted H_rho, b_rho.  M and S1 of the record stay plain.  The `out`
// and trace columns that hold sigma^2 hold F_rho.  No covariance.  Sizes and launch counts are the L2 entry points'.
extern "C" int pcl_gn_refine_l1(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                const float* rot, int pose_stride, int B, const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info,
                                float* trace, void* workspace, size_t workspace_bytes, float delta, void* stream)
{
    PclInfoL1 l1;
    if (!pcl_info_l1_args(delta, &l1)) return PCL_EINVAL;
    return pcl_gn_single<true>(cloud, weights, n, pano, pano_format, H, W, trans, rot, pose_stride, B, hyper_host, iters, state, out, info, nullptr, trace,
                               l1, workspace, workspace_bytes, stream);
}

extern "C" int pcl_gn_refine_images_l1(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets, const uint64_t* panos_host,
                                       int nimages, int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride,
                                       const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info, float* trace, void* workspace,
                                       size_t workspace_bytes, float delta, void* stream)
{
    PclInfoL1 l1;
    if (!pcl_info_l1_args(delta, &l1)) return PCL_EINVAL;
    return pcl_gn_images<true>(cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride, hyper_host,
                               iters, state, out, info, nullptr, trace, l1, workspace, workspace_bytes, stream);
}
