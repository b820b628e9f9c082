// pcl_gn.hip — a Levenberg-Marquardt polish of poses on the device, built on H and b of pcl_info.hip (additive to ABI 12).  BUILD-DEFINED:
// the reference refines with Adam and has nothing like it.
//
// What is minimised: the MEAN SQUARED residual sigma^2(theta) = sum w m l^2 / sum w m over theta = (t0, t1, t2, yaw, pitch, roll), with the
// Gauss-Newton model H = sum w m j j^T, b = sum w m l j of pcl_info.hip.  This is NOT the sampling loss sum w m l / sum w m that the GD chains
// minimise: the two share their per-point terms, mask and weights and are different objectives.  The mask m is treated as constant
// inside a step (it is re-evaluated at every trial pose).  Nothing is claimed about real data.
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

// (pcl_gn_step_rooms_kernel of pcl_gn_rooms.hip repeats this text over a room's region of rows.)
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_step_kernel(const float* __restrict__ partials, int nchunks, int B, PclGnState* __restrict__ state,
                                                               pcl_gn_hyper hp, int k, int iters, float* __restrict__ out, float* __restrict__ info,
                                                               float* __restrict__ cov, float* __restrict__ trace)
{
    __shared__ double s[PCL_INFO_ROW];
    __shared__ double A[6][6], C[6][6], T[6][6], Hm[6][6], L[6][6], Li[6][6], bv[6], dl[6];
    __shared__ float R[9];
    __shared__ double parts[PCL_BLOCK / PCL_INFO_ROW][PCL_INFO_ROW];
    const int b = blockIdx.x;
    PclGnState& st = state[b];
    if (st.frozen) return;                                           // (block-uniform: every thread leaves before the barriers)
    pcl_info_row_sum(partials, nchunks, B, b, parts, s);
    if (threadIdx.x != 0) return;

    double S2, S1, M, sigma2;
    const bool ok = pcl_info_chain(s, st.tri, st.tri + 3, A, C, T, Hm, bv, R, S2, S1, M, sigma2) && M > 0.0;
    const float F = (float)sigma2;
    const bool accept = ok && (k == 0 || F < st.F_acc);
    float lam = st.lam;
    bool freeze = false;
    st.evaluations += 1;
    if (accept || k == 0) {                                          // (k = 0 refused: its sums are what the record reports, status 1)
        for (int i = 0; i < 6; i++) {
            for (int m = 0; m < 6; m++) st.H[i][m] = Hm[i][m];
            st.b[i] = bv[i];
        }
        st.M = M; st.S1 = S1; st.S2 = S2; st.sums_ok = ok ? 1 : 0;
    }
    if (accept) {
        for (int i = 0; i < 6; i++) st.acc[i] = st.tri[i];
        st.F_acc = F;
        st.accepted += 1;
        if (k == 0) st.F_start = F;
        else lam = fmaxf(lam * hp.lam_down, hp.lam_min);
    } else {
        st.rejected += 1;
        if (k == 0) { st.status = 1; freeze = true; }
        else lam = fminf(lam * hp.lam_up, hp.lam_max);
    }
    st.lam = lam;
    if (trace) {
        float* tr = trace + ((int64_t)k * B + b) * PCL_GN_OUT;
        for (int i = 0; i < 6; i++) tr[i] = st.tri[i];
        tr[6] = F; tr[7] = accept ? 1.f : 0.f; tr[8] = lam; tr[9] = (float)M;
    }

    int e = 0;
    if (!freeze && k < iters) {
        // the step, on the accepted sums: D = H + lambda diag H in Hm, -b in bv
        for (int i = 0; i < 6; i++) {
            for (int m = 0; m < 6; m++) Hm[i][m] = st.H[i][m];
            Hm[i][i] = st.H[i][i] + (double)lam * st.H[i][i];
            bv[i] = -st.b[i];
        }
        if (pcl_info_factor(Hm, L, e) != 0) { st.status = 2; freeze = true; }
        else {
            // L y = -b, L^T z = y, delta = z / 2^e
            for (int i = 0; i < 6; i++) {
                double t = bv[i];
                for (int r = 0; r < i; r++) t -= L[i][r] * dl[r];
                dl[i] = t / L[i][i];
            }
            for (int i = 5; i >= 0; i--) {
                double t = dl[i];
                for (int r = i + 1; r < 6; r++) t -= L[r][i] * dl[r];
                dl[i] = t / L[i][i];
            }
            double mx = 0.0;
            for (int i = 0; i < 6; i++) { dl[i] = ldexp(dl[i], -e); mx = fmax(mx, fabs(dl[i])); }
            if (mx > (double)hp.step_cap) {
                const double sc = (double)hp.step_cap / mx;
                mx = 0.0;
                for (int i = 0; i < 6; i++) { dl[i] *= sc; mx = fmax(mx, fabs(dl[i])); }
            }
            bool same = true;
            for (int i = 0; i < 6; i++) {
                const float v = (float)((double)st.acc[i] + dl[i]);
                same = same && v == st.acc[i];
                st.tri[i] = v;
            }
            if (mx <= (double)hp.tol || same) { st.status = 3; freeze = true; }
        }
    }
    if (freeze) st.frozen = 1;
    if (!freeze && k < iters) return;

    // this pose is done: its outputs, from the accepted sums exactly as pcl_pose_information forms them
    float* o = out + (int64_t)b * PCL_GN_OUT;
    for (int i = 0; i < 6; i++) o[i] = st.acc[i];
    o[6] = st.F_start; o[7] = st.F_acc; o[8] = lam;
    o[9] = (float)st.accepted; o[10] = (float)st.rejected; o[11] = (float)st.evaluations; o[12] = (float)st.status;
    o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
    for (int i = 0; i < 6; i++) {
        for (int m = 0; m < 6; m++) Hm[i][m] = st.H[i][m];
        bv[i] = st.b[i];
    }
    M = st.M; S1 = st.S1; S2 = st.S2; sigma2 = S2 / M;
    int status = st.sums_ok ? 0 : 1;
    e = 0;
    if (status == 0) status = pcl_info_factor(Hm, L, e);
    pcl_info_emit(Hm, bv, M, S1, S2, sigma2, status, e, L, Li, info + (int64_t)b * PCL_INFO_REC, cov ? cov + (int64_t)b * 36 : nullptr);
}

int pcl_gn_launch_init(PclGnState* state, const float* trans, const float* rot, int pose_stride, float lam0, float* trace, int B, int iters, hipStream_t s)
{
    hipLaunchKernelGGL(pcl_gn_init_kernel, dim3((unsigned)B), dim3(PCL_BLOCK), 0, s, state, trans, rot, pose_stride, lam0, trace, B, iters);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t pcl_gn_state_bytes(int B)
{
    if (B <= 0) return 0;
    return pcl_align256((size_t)B * sizeof(PclGnState));
}

extern "C" size_t pcl_gn_workspace_bytes(int64_t n, int B)
{
    const int64_t nchunks = pcl_pass_chunks(n, PCL_INFO_MIN_STEPS, nullptr);
    if (nchunks == 0 || B <= 0 || nchunks * B > 0x7fffffffll) return 0;
    PclCarve c{nullptr, 0};
    c.take((size_t)nchunks * (size_t)B * PCL_INFO_ROW * sizeof(float));
    return c.off;
}

extern "C" int pcl_gn_refine(const float* cloud, const float* weights, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                             const float* rot, int pose_stride, int B, const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info,
                             float* cov, float* trace, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!hyper_host || !state || !out || !info || !workspace) return PCL_EINVAL;
    if (iters < 0 || iters > PCL_GN_MAX_ITERS || !pcl_gn_hyper_ok(hyper_host)) return PCL_EINVAL;
    PclInfoArgs a;
    int64_t nchunks;
    const int rc = pcl_pass_args(&a.pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, PCL_INFO_MIN_STEPS, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_gn_workspace_bytes(n, B)) return PCL_EINVAL;
    PclGnState* st = (PclGnState*)state;
    a.weights = weights; a.partials = (float*)workspace;
    a.pass.trans = st->tri; a.pass.rot = st->tri + 3; a.pass.pose_stride = (int)(sizeof(PclGnState) / sizeof(float));
    const pcl_gn_hyper hp = *hyper_host;
    const dim3 grid((unsigned)(nchunks * B)), blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pcl_gn_init_kernel, dim3((unsigned)B), blk, 0, s, st, trans, rot, pose_stride, hp.lam0, trace, B, iters);
    PCL_LAUNCH_CHECK();
    for (int k = 0; k <= iters; k++) {
        pcl_with_flag(weights != nullptr, [&](auto wt) {
            pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                hipLaunchKernelGGL((pcl_gn_pass_kernel<decltype(fmt)::value, decltype(wt)::value>), grid, blk, 0, s, a, (const PclGnState*)st);
            });
        });
        PCL_LAUNCH_CHECK();
        hipLaunchKernelGGL(pcl_gn_step_kernel, dim3((unsigned)B), blk, 0, s, (const float*)a.partials, (int)nchunks, B, st, hp, k, iters, out, info, cov, trace);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// pcl_gn_refine for nimages poses, each against ITS OWN panorama, colour set and weight plane, in one chain: the init and step launches run
// over all the images (they are per pose and do not care which image a pose belongs to), the gated pass runs once per
// PCL_RES_MAX_IMAGES images into the call's [nchunks][nimages] partial rows.  1 + (groups + 1) (iters + 1) launches.
extern "C" int pcl_gn_refine_images(const float* cloud, const float* weights, int weight_sets, int64_t n, int color_sets, const uint64_t* panos_host,
                                    int nimages, int pano_format, int H, int W, const float* trans, const float* rot, int pose_stride,
                                    const pcl_gn_hyper* hyper_host, int iters, void* state, float* out, float* info, float* cov, float* trace,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    if (!hyper_host || !state || !out || !info || !workspace) return PCL_EINVAL;
    if (iters < 0 || iters > PCL_GN_MAX_ITERS || !pcl_gn_hyper_ok(hyper_host)) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    int64_t nchunks;
    const int rc = pcl_info_images_args(&a, &im, cloud, weights, weight_sets, n, color_sets, panos_host, nimages, pano_format, H, W, trans, rot,
                                        pose_stride, &nchunks);
    if (rc) return rc;
    if (workspace_bytes < pcl_gn_workspace_bytes(n, nimages)) return PCL_EINVAL;
    PclGnState* st = (PclGnState*)state;
    a.partials = (float*)workspace;
    a.pass.trans = st->tri; a.pass.rot = st->tri + 3; a.pass.pose_stride = (int)(sizeof(PclGnState) / sizeof(float));
    const pcl_gn_hyper hp = *hyper_host;
    const dim3 blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pcl_gn_init_kernel, dim3((unsigned)nimages), blk, 0, s, st, trans, rot, pose_stride, hp.lam0, trace, nimages, iters);
    PCL_LAUNCH_CHECK();
    for (int k = 0; k <= iters; k++) {
        pcl_info_images_launches(a, im, panos_host, nchunks, [&](const PclInfoArgs& al, const PclInfoImages& il, int i0, dim3 grid) {
            pcl_with_flag(weights != nullptr, [&](auto wt) {
                pcl_with_flag(color_sets > 1, [&](auto cs) {
                    pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                        hipLaunchKernelGGL((pcl_gn_pass_images_kernel<decltype(fmt)::value, decltype(wt)::value, decltype(cs)::value>), grid, blk, 0, s,
                                           al, il, (const PclGnState*)(st + i0));
                    });
                });
            });
        });
        PCL_LAUNCH_CHECK();
        hipLaunchKernelGGL(pcl_gn_step_kernel, dim3((unsigned)nimages), blk, 0, s, (const float*)a.partials, (int)nchunks, nimages, st, hp, k, iters, out,
                           info, cov, trace);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

