// pcl_gn_step_body.h — the body of the step kernels of the Levenberg-Marquardt chain, pcl_gn_step_kernel (pcl_gn.hip) and
// pcl_gn_step_rooms_kernel (pcl_gn_rooms.hip): a TEXT, #included inside each kernel after a prologue, not a header (no include guard).
// The prologue defines the names the text reads beside the kernels' common parameters (state, hp, k, iters, out, info, cov, trace):
//   int B, b                                       pose b of the call's B: state[b], out / info / cov row b, trace row k * B + b
//   const float* partials; int nchunks, rowsB, row the pose's chunk rows are partials[(c * rowsB + row) * PCL_INFO_ROW ..], c < nchunks
//                                                  (single and images chains: rowsB = B, row = b; rooms: the room's region, its image count
//                                                  and the pose's image)
// Why a text and not a function: as a forced-inline device function called by both kernels (with or without __restrict__ on its
// parameters) this body compiles to another instruction stream in BOTH of them (3496 -> 3599 and 3542 -> 3642 listing lines), and the
// sign bits of the NaNs that a pose which is not finite reports depend on that stream; included as text, both kernels keep the listing
// they had when each spelled the body out.
// The algebra is that of the device functions of pcl_info_device.h (row sum, chain rule, factorisation, record); the finish kernels of
// pcl_info.hip have the same algebra as one monolithic text, pcl_info_finish_body.h.  That the two agree bit for bit is asserted on
// the device, by the tests.
    __shared__ double s[PCL_INFO_ROW];
    __shared__ double A[6][6], C[6][6], T[6][6], Hm[6][6], L[6][6], Li[6][6], bv[6], dl[6];
    __shared__ float R[9];
    __shared__ double parts[PCL_BLOCK / PCL_INFO_ROW][PCL_INFO_ROW];
    PclGnState& st = state[b];
    if (st.frozen) return;                                           // (block-uniform: every thread leaves before the barriers)
    pcl_info_row_sum(partials, nchunks, rowsB, row, parts, s);
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
