// pcl_gn_rooms.hip — the Levenberg-Marquardt polish of pcl_gn.hip for the winners of a rooms x images chain (additive to ABI 12; BUILD-DEFINED):
// pose (r, i) = row r * nimages + i against room r's cloud, panorama i and colour set i of room r, every room over its own chunking and its
// own region of partial rows.  The per-point pass is pcl_info_pass_at of pcl_info_device.h behind pcl_gn_pass_kernel's gate, the step is
// pcl_gn_step_kernel's text: record (r, i) has the bits of pcl_gn_refine of that pose, cloud, colour set and panorama alone.
#include <math.h>

#include "pcl_gn_device.h"

// The pass of pcl_gn_refine_rooms: pcl_pose_info_rooms_kernel's block behind the gate of its own pose (r, i); `state` is that of the launch's
// first image in room 0, rows r * btot + i apart like the poses read from it.
template <int FMT, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_rooms_kernel(PclInfoArgs a, PclInfoImages im, PclInfoRooms rm, const PclGnState* __restrict__ state)
{
    const PclInfoRoomAt at = pcl_info_room_select(rm, (unsigned)a.pass.B);
    if (state[at.room * (unsigned)im.btot + at.image].frozen) return;      // (a scalar load: the address depends on the block alone)
    pcl_info_pass_rooms<FMT, CS>(a, im, at);
}

// The step of pcl_gn_refine_rooms: one block per pose (r, i) = blockIdx.x of B = nrooms * nimages, over room r's region and chunk count.
// pcl_gn_step_kernel's text, statement for statement (see pcl_pose_info_finish_rooms_kernel: the sign bits of the NaNs a pose that is not
// finite reports depend on the statements' form).
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_step_rooms_kernel(const float* __restrict__ partials_all, PclInfoRooms rm, int nimages, int B,
                                                                     PclGnState* __restrict__ state, pcl_gn_hyper hp, int k, int iters,
                                                                     float* __restrict__ out, float* __restrict__ info, float* __restrict__ cov,
                                                                     float* __restrict__ trace)
{
    __shared__ double s[PCL_INFO_ROW];
    __shared__ double A[6][6], C[6][6], T[6][6], Hm[6][6], L[6][6], Li[6][6], bv[6], dl[6];
    __shared__ float R[9];
    __shared__ double parts[PCL_BLOCK / PCL_INFO_ROW][PCL_INFO_ROW];
    const int b = blockIdx.x, room = b / nimages;
    const float* __restrict__ partials = partials_all + rm.rec[room].rows;
    const int nchunks = rm.rec[room].nchunks;
    PclGnState& st = state[b];
    if (st.frozen) return;                                           // (block-uniform: every thread leaves before the barriers)
    pcl_info_row_sum(partials, nchunks, nimages, b - room * nimages, parts, s);
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

extern "C" size_t pcl_gn_rooms_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int nimages)
{
    PclInfoRoomsPlan g;
    return pcl_info_rooms_plan(rooms_host, nrooms, nimages, &g) ? 0 : g.bytes;
}

// pcl_gn_refine for the nrooms * nimages poses (r, i), each against room r's cloud, colour set i and panos_host[i], in one chain: the init
// launch runs over all poses as it is, the gated rooms pass once per PCL_RES_MAX_IMAGES images over all rooms, the rooms step over all
// poses.  1 + (groups + 1) (iters + 1) launches.
extern "C" int pcl_gn_refine_rooms(const pcl_gd_room* rooms_host, int nrooms, int color_sets, const uint64_t* panos_host, int nimages, int pano_format,
                                   int H, int W, const float* trans, const float* rot, int pose_stride, const pcl_gn_hyper* hyper_host, int iters,
                                   void* state, float* out, float* info, float* cov, float* trace, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!hyper_host || !state || !out || !info || !workspace) return PCL_EINVAL;
    if (iters < 0 || iters > PCL_GN_MAX_ITERS || !pcl_gn_hyper_ok(hyper_host)) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    PclInfoRoomsPlan g;
    const int rc = pcl_info_rooms_args(&a, &im, &g, rooms_host, nrooms, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride);
    if (rc) return rc;
    if (workspace_bytes < g.bytes) return PCL_EINVAL;
    const int B = nrooms * nimages;
    PclGnState* st = (PclGnState*)state;
    a.partials = (float*)workspace;
    a.pass.trans = st->tri; a.pass.rot = st->tri + 3; a.pass.pose_stride = (int)(sizeof(PclGnState) / sizeof(float));
    const pcl_gn_hyper hp = *hyper_host;
    const dim3 blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    const int rci = pcl_gn_launch_init(st, trans, rot, pose_stride, hp.lam0, trace, B, iters, s);
    if (rci) return rci;
    for (int k = 0; k <= iters; k++) {
        pcl_info_rooms_launches(a, im, g, panos_host, [&](const PclInfoArgs& al, const PclInfoImages& il, const PclInfoRooms& tl, int i0, dim3 grid) {
            pcl_with_flag(color_sets > 1, [&](auto cs) {
                pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                    hipLaunchKernelGGL((pcl_gn_pass_rooms_kernel<decltype(fmt)::value, decltype(cs)::value>), grid, blk, 0, s, al, il, tl,
                                       (const PclGnState*)(st + i0));
                });
            });
        });
        PCL_LAUNCH_CHECK();
        hipLaunchKernelGGL(pcl_gn_step_rooms_kernel, dim3((unsigned)B), blk, 0, s, (const float*)a.partials, g.t, nimages, B, st, hp, k, iters, out, info,
                           cov, trace);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}
