// pcl_info_finish_body.h — the body of the finish kernels of pcl_info.hip, pcl_pose_info_finish_kernel and pcl_pose_info_finish_rooms_kernel:
// a TEXT, #included inside each kernel after a prologue, not a header (no include guard: it is included once per kernel).
// The prologue defines the names the text reads:
//   const float* partials; int nchunks, B, b     pose b's chunk rows are partials[(c * B + b) * PCL_INFO_ROW ..], c < nchunks
//   const float* trans, rot; int pose_stride      pose b is at trans / rot + b * pose_stride
//   float* info, cov                              record b at info + b * PCL_INFO_REC, covariance b at cov + b * 36 (cov may be null)
// Why a text and not a function: as a forced-inline device function called by both kernels this body compiles to another instruction
// stream in BOTH of them (3291 -> 2695 and 3365 -> 2770 listing lines), and a pose that is not finite then reports NaNs with other
// sign bits; included as text, both kernels keep the listing they had when each spelled the body out.
//
// One 256-thread block per pose.  Thread (part, k), part = tid / 32, adds entry k of its eighth of the chunks' rows in double, lowest chunk
// first; the eight parts are then added pairwise in a fixed order (a 1M-point cloud has ~1000 rows per pose: one lane walking them all
// is most of the call's time at B = 1).  Thread 0 then does the 6 x 6 algebra in double on matrices kept in LDS (runtime indices there
// cost nothing; in registers they would cost scratch) and rounds every output once.
//   j = C a:  grad_t = -R^T g;  yaw = tau_z;  pitch = -sy tau_x + cy tau_y;  roll = cy cp tau_x + sy cp tau_y - sp tau_z
// with R the fp32 matrix of pcl_rot_from_ypr and the sines / cosines of the fp32 angles in double, as pcl_finish_kernel takes them.
// The factorisation runs on H scaled by an exact power of two (largest diagonal entry into [1/2, 1)), so that weights scaled by a power
// of two scale cov by the inverse power and change no other bit.  status 2: a pivot <= 6 * 2^-52 * (the largest diagonal entry).
// (pcl_info_device.h restates the row sum, the chain rule, the factorisation and the record as device functions for the step text,
// pcl_gn_step_body.h; this text, built from those functions, computes the same and compiles to another instruction stream.  That the two
// agree bit for bit is asserted on the device, by the tests.)
    __shared__ double s[PCL_INFO_ROW];
    __shared__ double A[6][6], C[6][6], T[6][6], Hm[6][6], L[6][6], Li[6][6], bv[6];
    __shared__ float R[9];
    __shared__ double parts[PCL_BLOCK / PCL_INFO_ROW][PCL_INFO_ROW];
    const int k = threadIdx.x % PCL_INFO_ROW, part = threadIdx.x / PCL_INFO_ROW;
    {
        const int per = (nchunks + PCL_BLOCK / PCL_INFO_ROW - 1) / (PCL_BLOCK / PCL_INFO_ROW);
        const int c0 = part * per, c1 = min(nchunks, c0 + per);
        double t = 0.0;
        for (int c = c0; c < c1; c++) t += (double)partials[((int64_t)c * B + b) * PCL_INFO_ROW + k];
        parts[part][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < PCL_INFO_ROW)
        s[k] = ((parts[0][k] + parts[1][k]) + (parts[2][k] + parts[3][k])) + ((parts[4][k] + parts[5][k]) + (parts[6][k] + parts[7][k]));
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float* tp = trans + (int64_t)b * pose_stride;
    const float* rp = rot + (int64_t)b * pose_stride;
    double sy, cy, sp, cp;
    sincos((double)rp[0], &sy, &cy);
    sincos((double)rp[1], &sp, &cp);
    pcl_rot_from_ypr(rp[0], rp[1], rp[2], R);
    bool finite = true;
    for (int i = 0; i < 3; i++) finite = finite && fabsf(tp[i]) <= 3.402823466e38f && fabsf(rp[i]) <= 3.402823466e38f;
    for (int i = 0; i < 6; i++)
        for (int m = 0; m < 6; m++) C[i][m] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int m = 0; m < 3; m++) C[i][m] = -(double)R[3 * m + i];
    C[3][5] = 1.0;
    C[4][3] = -sy; C[4][4] = cy;
    C[5][3] = cy * cp; C[5][4] = sy * cp; C[5][5] = -sp;
    int q = 0;
    for (int i = 0; i < 6; i++)
        for (int m = i; m < 6; m++, q++) { A[i][m] = s[q]; A[m][i] = s[q]; }
    for (int i = 0; i < 6; i++)
        for (int m = 0; m < 6; m++) {
            double t = 0.0;
            for (int r = 0; r < 6; r++) t += C[i][r] * A[r][m];
            T[i][m] = t;
        }
    for (int i = 0; i < 6; i++) {
        for (int m = i; m < 6; m++) {
            double t = 0.0;
            for (int r = 0; r < 6; r++) t += T[i][r] * C[m][r];
            Hm[i][m] = t; Hm[m][i] = t;
        }
        double t = 0.0;
        for (int r = 0; r < 6; r++) t += C[i][r] * s[21 + r];
        bv[i] = t;
    }
    const double S2 = s[27], S1 = s[28], M = s[29], sigma2 = S2 / M;
    for (int i = 0; i < PCL_INFO_NSUM; i++) finite = finite && fabs(s[i]) <= 1.7976931348623157e308;
    for (int i = 0; i < 6; i++) {
        finite = finite && fabs(bv[i]) <= 1.7976931348623157e308;
        for (int m = 0; m < 6; m++) finite = finite && fabs(Hm[i][m]) <= 1.7976931348623157e308;
    }
    int status = (finite && M > 0.0) ? 0 : 1;
    int e = 0;
    if (status == 0) {
        double maxd = 0.0;
        for (int i = 0; i < 6; i++) maxd = fmax(maxd, Hm[i][i]);
        if (!(maxd > 0.0)) status = 2;
        else {
            const double ms = frexp(maxd, &e), tol = 6.0 * 2.220446049250313e-16 * ms;
            for (int i = 0; i < 6 && status == 0; i++) {
                double d = ldexp(Hm[i][i], -e);
                for (int r = 0; r < i; r++) d -= L[i][r] * L[i][r];
                if (!(d > tol)) { status = 2; break; }
                const double piv = sqrt(d);
                L[i][i] = piv;
                for (int m = i + 1; m < 6; m++) {
                    double t = ldexp(Hm[m][i], -e);
                    for (int r = 0; r < i; r++) t -= L[m][r] * L[i][r];
                    L[m][i] = t / piv;
                }
            }
        }
    }
    float* o = info + (int64_t)b * PCL_INFO_REC;
    for (int i = 0; i < 6; i++)
        for (int m = 0; m < 6; m++) o[6 * i + m] = (float)Hm[i][m];
    for (int i = 0; i < 6; i++) o[36 + i] = (float)bv[i];
    o[42] = (float)M; o[43] = (float)S1; o[44] = (float)S2; o[45] = (float)sigma2; o[46] = (float)status; o[47] = 0.f;
    if (!cov) return;
    float* cv = cov + (int64_t)b * 36;
    if (status != 0) {
        for (int i = 0; i < 36; i++) cv[i] = __builtin_nanf("");
        return;
    }
    // Li = L^-1 (lower triangular), (H / 2^e)^-1 = Li^T Li
    for (int m = 0; m < 6; m++) {
        Li[m][m] = 1.0 / L[m][m];
        for (int i = m + 1; i < 6; i++) {
            double t = 0.0;
            for (int r = m; r < i; r++) t += L[i][r] * Li[r][m];
            Li[i][m] = -t / L[i][i];
        }
    }
    for (int i = 0; i < 6; i++)
        for (int m = i; m < 6; m++) {
            double t = 0.0;
            for (int r = m; r < 6; r++) t += Li[r][i] * Li[r][m];
            const float c = (float)ldexp(sigma2 * t, -e);
            cv[6 * i + m] = c; cv[6 * m + i] = c;
        }
