// pcl_info_device.h — what pcl_info.hip (the information matrix at given poses) and pcl_gn.hip (the Levenberg-Marquardt chain on it) share:
// the per-point pass that accumulates the 30 sums into one partial row per (chunk, pose), the fixed-order sum of a pose's rows in
// double, the chain rule H = C A C^T, b = C v, the Cholesky factorisation on a power-of-two scaling and the info record / covariance.
// Every function is inlined into its kernel: a kernel built from them has the arithmetic, and the bits, of every other.  The step text
// (pcl_gn_step_body.h) is built from the row sum, chain rule, factorisation and record below; the finish text (pcl_info_finish_body.h)
// spells the same algebra out on its own, because built from these functions it compiles to another instruction stream.  An edit to
// the algebra is made in those two places, here and there, and the tests assert on the device that they agree bit for bit.
// Outside the loss-kernel hash: the four files it covers are included, never edited.
#pragma once
#include <math.h>
#include <string.h>

#include "pcl_point_pass.h"
#include "pcl_sample_device.h"

#define PCL_INFO_MIN_STEPS 2               // a chunk walks at least two steps where the cloud has them (a one-off call: fewer, longer blocks)
#define PCL_INFO_ROW 32                    // floats per partial row: A (21, k <= l row-major), sum w l a (6), S2, S1, M, 0, 0
#define PCL_INFO_NSUM 30
#define PCL_INFO_REC 48                    // floats per info record (include/piccolo_hip.h)

struct PclInfoArgs {
    PclPassArgs pass;
    const float* weights;    // WT: one more plane of `stride` floats, packed order (the images instances: one per image, back to back)
    float* partials;         // [nchunks][B][PCL_INFO_ROW] (the images instances: B = the call's image count)
};

// What the images instances (pose b against panorama b) take beside PclInfoArgs: this launch's panorama addresses, and where the launch
// sits in its call — a.pass.B is the LAUNCH's pose count, `img0` its first image, `btot` the call's image count (the partial rows are
// [nchunks][btot]), `sets` the cloud's colour sets and `wsets` the weight resource's planes (1: one plane for every image).
struct PclInfoImages {
    PclResPanos panos;
    int sets, img0, btot, wsets;
};

// The whole per-point pass of a block: the pass of pcl_point_pass.h with the weighted gradient instance of pcl_sample2 under UNIT weight,
// the 30 packed-fp32 accumulators, and the block's sums in a fixed order into partial row `row`.  The block's panorama is `pano_b`; with
// CS it reads colour set `set` of `sets`; with WT the weight resource covers `wsets` planes of `stride` floats and the block reads the
// one at byte offset `wplane`, which goes through the load's scalar offset (wave-uniform), as the loss kernel's wsets instances do it.
// The single-image kernels pass a.pass.pano, one set, one plane at offset 0 and row blockIdx.x as literals: their instruction streams
// are those of the pass before it took these arguments.
// pcl_info_pass_at is that pass for block (chunk, pose b) over the cloud `c` into row `row` of `partials`: what a block of a rooms launch
// passes from its room's record, and what pcl_info_pass passes from the call's own struct and block index.
// With L1 (the Huber-L1 form of the polish, pcl_gn.hip) a pair's factor on the 21 + 6 moment sums is w phi(l), phi = min(1 / l, 1 / delta)
// (v_rcp_f32; l = 0: 1 / delta, and a masked point's a = 0 anyway), slot 27 takes sum w rho(l), rho = l >= delta ? l - delta / 2 :
// l^2 / (2 delta), in place of S2, and S1 and M keep the plain w.  inv_delta = 1 / delta and half_delta = delta / 2 are formed on the host
// and travel by value in the kernel arguments (wave-uniform: SGPRs); delta itself is half_delta + half_delta, exactly.  Without L1 the two
// are not read and the instruction stream is the one it was before the flag.
// With DEPTH (pcl_depth_info.hip) the pass is pcl_point_pass_at's depth form over the z-buffers `dz`: a hidden point arrives with l = 0,
// m = 0 and a = 0 like a masked one and adds nothing to any sum; the two visibility bits are not needed here.  Without it: as before.
template <int FMT, bool WT, bool CS = false, bool L1 = false, bool DEPTH = false>
__device__ __forceinline__ void pcl_info_pass_at(const PclInfoArgs& a, const PclPassCloud& c, unsigned b, unsigned chunk, const void* pano_b, int sets,
                                                 unsigned set, int wsets, int wplane, float* partials, unsigned row, float inv_delta = 0.f,
                                                 float half_delta = 0.f, const PclPassDepth* dz = nullptr)
{
    __amdgpu_buffer_rsrc_t wrs;
    if constexpr (WT) wrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.weights, 0, (int)(c.stride * 4) * wsets, 0x00020000);

    f2 hh[21], bb[6], s2 = F2(0.f), s1 = F2(0.f), mm = F2(0.f);
#pragma unroll
    for (int k = 0; k < 21; k++) hh[k] = F2(0.f);
#pragma unroll
    for (int k = 0; k < 6; k++) bb[k] = F2(0.f);

    // (auto...: the depth form's two visibility bits, not read)
    pcl_point_pass_at<FMT, true, CS, DEPTH>(a.pass, c, b, chunk, pano_b, sets, set, [&](int, int j, bool valid0, bool valid1, const f2* acc, bool, auto...) {
        // acc: 0 l, 1 m, 2-4 g, 5-7 tau of this pair of points alone.  One factor w (a slot past n never counts, whatever its plane holds)
        f2 w = F2(1.f), wl = acc[0], wm = acc[1], wa[6];
        if constexpr (WT) {
            w = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(wrs, j * 4, wplane, 0));
            w = (f2){valid0 ? w.x : 0.f, valid1 ? w.y : 0.f};
            wl = w * acc[0]; wm = w * acc[1];
        }
        if constexpr (L1) {
            // the IRLS weight of the pair: the saturated branch is the host's 1 / delta itself
            const f2 phi = (f2){fminf(__builtin_amdgcn_rcpf(acc[0].x), inv_delta), fminf(__builtin_amdgcn_rcpf(acc[0].y), inv_delta)};
            const f2 wp = WT ? w * phi : phi;
#pragma unroll
            for (int k = 0; k < 6; k++) wa[k] = wp * acc[2 + k];
        } else {
#pragma unroll
            for (int k = 0; k < 6; k++) wa[k] = WT ? w * acc[2 + k] : acc[2 + k];
        }
        int q = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int l = k; l < 6; l++, q++) hh[q] = pcl_fma2(wa[k], acc[2 + l], hh[q]);
        }
#pragma unroll
        for (int k = 0; k < 6; k++) bb[k] = pcl_fma2(wa[k], acc[0], bb[k]);
        if constexpr (L1) {
            const float delta = half_delta + half_delta, hi = 0.5f * inv_delta;
            const f2 l = acc[0];
            const f2 rho = (f2){l.x >= delta ? l.x - half_delta : l.x * l.x * hi, l.y >= delta ? l.y - half_delta : l.y * l.y * hi};
            if constexpr (WT) s2 = pcl_fma2(w, rho, s2);
            else s2 += rho;
        } else {
            s2 = pcl_fma2(wl, acc[0], s2);
        }
        s1 += wl;
        mm += wm;
    }, dz);

    // the block's sums in a fixed order: packed halves, the lanes of a wave (DPP), the four waves (LDS)
    __shared__ float red[PCL_BLOCK / PCL_WAVE][PCL_INFO_ROW];
    const int lane = threadIdx.x & (PCL_WAVE - 1), wave = threadIdx.x / PCL_WAVE;
    auto put = [&](int k, f2 t) {
        const float r = pcl_wave_sum(t.x + t.y);
        if (lane == 0) red[wave][k] = r;
    };
#pragma unroll
    for (int k = 0; k < 21; k++) put(k, hh[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) put(21 + k, bb[k]);
    put(27, s2); put(28, s1); put(29, mm);
    if (lane == 0) { red[wave][30] = 0.f; red[wave][31] = 0.f; }
    __syncthreads();
    if (threadIdx.x < PCL_INFO_ROW) {
        const int k = threadIdx.x;
        partials[(int64_t)row * PCL_INFO_ROW + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

template <int FMT, bool WT, bool CS = false, bool L1 = false>
__device__ __forceinline__ void pcl_info_pass(const PclInfoArgs& a, const void* pano_b, int sets, unsigned set, int wsets, int wplane, unsigned row,
                                              float inv_delta = 0.f, float half_delta = 0.f)
{
    pcl_info_pass_at<FMT, WT, CS, L1>(a, PclPassCloud{a.pass.cloud, a.pass.n, a.pass.stride, a.pass.steps_base, a.pass.steps_rem},
                                      blockIdx.x % (unsigned)a.pass.B, blockIdx.x / (unsigned)a.pass.B, pano_b, sets, set, wsets, wplane, a.partials, row,
                                      inv_delta, half_delta);
}

// ---- host side of the objective.  The host body of a form in pcl_info.hip and pcl_gn.hip is a template over `bool L1` that takes a PclInfoL1
// by value and reads it under L1 only; the L2 and the L1 entry point of the form are its two instances.  (A template and not a runtime
// flag: the instances are made in the order of the entry points, and a translation unit emits its kernels in the order it always did.)
// delta is refused unless it is finite and inside [2^-20, 4] as a float (residuals never exceed sqrt(3); the range keeps 1 / delta and
// what it scales well inside fp32)
struct PclInfoL1 {
    float inv_delta, half_delta;
};
static inline bool pcl_info_l1_args(float delta, PclInfoL1* l1)
{
    if (!(delta >= 9.5367431640625e-07f && delta <= 4.f)) return false;      // (a NaN fails both)
    l1->inv_delta = 1.f / delta; l1->half_delta = 0.5f * delta;
    return true;
}

// ---- the rooms instances (pcl_pose_information_rooms, pcl_gn_refine_rooms): pose (r, i) = row r * btot + i against room r's cloud,
// panorama i and, with CS, colour set i of room r's cloud.  Room r owns the contiguous blocks [block0_r, block0_r + nchunks_r * m) of a
// launch of m images, the image varying fastest, walks its own chunking pcl_pass_chunks(n_r, PCL_INFO_MIN_STEPS), and keeps its partial
// rows [nchunks_r][btot][PCL_INFO_ROW] in a region of its own, `rows` floats into the call's partials.  The table travels as kernel
// arguments: a block counts the rooms that start at or before it (unused entries of block0 hold INT_MAX) and reads its record with
// scalar loads at an index that depends on the block index alone — everything below is wave-uniform and lives in SGPRs, the cloud's
// buffer resource included.
struct PclInfoRoom {
    unsigned long long cloud;      // packed cloud of the room (pcl_cloud_pack / pcl_cloud_pack_sets)
    long long rows;                // float offset of the room's partial rows
    int n, stride;
    int nchunks, block0;           // block0: of this LAUNCH (it depends on the launch's image count)
    int steps_base, steps_rem;
};
struct PclInfoRooms {
    int block0[PCL_GD_MAX_ROOMS];
    PclInfoRoom rec[PCL_GD_MAX_ROOMS];
};

__device__ __forceinline__ int pcl_info_sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long pcl_info_sgpr64(unsigned long long v)
{
    return ((unsigned long long)(unsigned)pcl_info_sgpr((int)(v >> 32)) << 32) | (unsigned long long)(unsigned)pcl_info_sgpr((int)(unsigned)v);
}

// Where block blockIdx.x of a rooms launch of `m` images works: its room, the room's cloud and chunking, its chunk and its image
struct PclInfoRoomAt {
    PclPassCloud c;
    unsigned room, chunk, image;
    long long rows;
};
__device__ __forceinline__ PclInfoRoomAt pcl_info_room_select(const PclInfoRooms& rm, unsigned m)
{
    int r = -1;
#pragma unroll
    for (int q = 0; q < PCL_GD_MAX_ROOMS; q++) r += (int)blockIdx.x >= rm.block0[q] ? 1 : 0;
    r = pcl_info_sgpr(r);
    const PclInfoRoom& e = rm.rec[r];
    const unsigned local = blockIdx.x - (unsigned)pcl_info_sgpr(e.block0);
    PclInfoRoomAt at;
    at.c = PclPassCloud{(const float*)pcl_info_sgpr64(e.cloud), (int64_t)pcl_info_sgpr(e.n), (int64_t)pcl_info_sgpr(e.stride), pcl_info_sgpr(e.steps_base),
                        pcl_info_sgpr(e.steps_rem)};
    at.room = (unsigned)r; at.chunk = local / m; at.image = local - at.chunk * m;
    at.rows = (long long)pcl_info_sgpr64((unsigned long long)e.rows);
    return at;
}

// The block of the rooms pass launches: pose at.room * btot + at.image of the launch's sliced poses against panorama at.image of the launch,
// colour set img0 + at.image, into row chunk * btot + img0 + at.image of the room's region.  No weights: the rooms chains take none.
template <int FMT, bool CS>
__device__ __forceinline__ void pcl_info_pass_rooms(const PclInfoArgs& a, const PclInfoImages& im, const PclInfoRoomAt& at)
{
    const unsigned g = at.image + (unsigned)im.img0;
    pcl_info_pass_at<FMT, false, CS>(a, at.c, at.room * (unsigned)im.btot + at.image, at.chunk, (const void*)im.panos.p[at.image], im.sets, g, 1, 0,
                                     a.partials + at.rows, at.chunk * (unsigned)im.btot + g);
}

// All 256 threads of a block.  Thread (part, k), part = tid / 32, adds entry k of its eighth of pose b's chunk rows in double, lowest chunk
// first; the eight parts are then added pairwise in a fixed order into s[k] (a 1M-point cloud has ~1000 rows per pose: one lane walking
// them all is most of a call's time at B = 1).  s is complete after the second barrier.
__device__ __forceinline__ void pcl_info_row_sum(const float* __restrict__ partials, int nchunks, int B, int b, double (*parts)[PCL_INFO_ROW], double* s)
{
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
}

// One thread, matrices in LDS (runtime indices there cost nothing; in registers they would cost scratch).  H = C A C^T and b = C v in
// double from the sums s at the pose (tp, rp):
//   j = C a:  grad_t = -R^T g;  yaw = tau_z;  pitch = -sy tau_x + cy tau_y;  roll = cy cp tau_x + sy cp tau_y - sp tau_z
// with R the fp32 matrix of pcl_rot_from_ypr and the sines / cosines of the fp32 angles in double, as pcl_finish_kernel takes them.
// -> whether the pose, the 30 sums, H and b are all finite; S2, S1, M and sigma^2 = S2 / M
__device__ __forceinline__ bool pcl_info_chain(const double* s, const float* tp, const float* rp, double (*A)[6], double (*C)[6], double (*T)[6],
                                               double (*Hm)[6], double* bv, float* R, double& S2, double& S1, double& M, double& sigma2)
{
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
    S2 = s[27]; S1 = s[28]; M = s[29]; sigma2 = S2 / M;
    for (int i = 0; i < PCL_INFO_NSUM; i++) finite = finite && fabs(s[i]) <= 1.7976931348623157e308;
    for (int i = 0; i < 6; i++) {
        finite = finite && fabs(bv[i]) <= 1.7976931348623157e308;
        for (int m = 0; m < 6; m++) finite = finite && fabs(Hm[i][m]) <= 1.7976931348623157e308;
    }
    return finite;
}

// Cholesky factor L of Hm scaled by an exact power of two, 2^-e (largest diagonal entry into [1/2, 1)), so that a matrix scaled by a power
// of two has the same L bit for bit.  -> 0, or 2: a pivot <= 6 * 2^-52 * (the largest diagonal entry)
__device__ __forceinline__ int pcl_info_factor(const double (*Hm)[6], double (*L)[6], int& e)
{
    int status = 0;
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
    return status;
}

// The 48-float info record o and (cv != nullptr) the covariance sigma^2 H^-1 from the factor L of H / 2^e, every output rounded once
__device__ __forceinline__ void pcl_info_emit(const double (*Hm)[6], const double* bv, double M, double S1, double S2, double sigma2, int status, int e,
                                              const double (*L)[6], double (*Li)[6], float* o, float* cv)
{
    for (int i = 0; i < 6; i++)
        for (int m = 0; m < 6; m++) o[6 * i + m] = (float)Hm[i][m];
    for (int i = 0; i < 6; i++) o[36 + i] = (float)bv[i];
    o[42] = (float)M; o[43] = (float)S1; o[44] = (float)S2; o[45] = (float)sigma2; o[46] = (float)status; o[47] = 0.f;
    if (!cv) return;
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
}

// ---- host side: the partial rows [nchunks][B][PCL_INFO_ROW] of a call over one cloud, which are the whole workspace of
// pcl_pose_information, pcl_pose_information_images, pcl_gn_refine and pcl_gn_refine_images (0: n or B out of range, or more blocks than
// a grid holds)
static inline size_t pcl_info_workspace_bytes(int64_t n, int B)
{
    const int64_t nchunks = pcl_pass_chunks(n, PCL_INFO_MIN_STEPS, nullptr);
    if (nchunks == 0 || B <= 0 || nchunks * B > 0x7fffffffll) return 0;
    PclCarve c{nullptr, 0};
    c.take((size_t)nchunks * (size_t)B * PCL_INFO_ROW * sizeof(float));
    return c.off;
}

// pcl_pose_info_finish_kernel over B poses (pcl_info.hip): the one place that launches it, for the bodies of pcl_info.hip and the entry
// point of pcl_depth_info.hip
int pcl_info_launch_finish(const float* partials, int nchunks, int B, const float* trans, const float* rot, int pose_stride, float* info, float* cov,
                           hipStream_t s);

// ---- host side of the images entry points (pcl_pose_information_images, pcl_gn_refine_images): every check, before any launch
// weights == NULL with weight_sets 0; else weight_sets 1 (one plane for every image) or nimages (plane i at weights + i * stride);
// color_sets 0 / 1 (the cloud's one set) or nimages (pcl_point_residuals_images' rule).  Fills a (a.pass.B = nimages, a.pass.pano = the
// first panorama) and what the launches of one call share of im; a launch sets im->panos, im->img0 and its own pose count.
static inline int pcl_info_images_args(PclInfoArgs* a, PclInfoImages* im, const float* cloud, const float* weights, int weight_sets, int64_t n,
                                       int color_sets, const uint64_t* panos_host, int nimages, int pano_format, int H, int W, const float* trans,
                                       const float* rot, int pose_stride, int64_t* nchunks_out)
{
    if (!panos_host || nimages <= 0) return PCL_EINVAL;
    for (int i = 0; i < nimages; i++)
        if (!panos_host[i]) return PCL_EINVAL;
    if (weights ? (weight_sets != 1 && weight_sets != nimages) : weight_sets != 0) return PCL_EINVAL;
    if (color_sets < 0 || (color_sets > 1 && color_sets != nimages)) return PCL_EINVAL;
    const int rc = pcl_pass_args(&a->pass, cloud, n, (const void*)panos_host[0], pano_format, H, W, trans, rot, pose_stride, nimages, PCL_INFO_MIN_STEPS,
                                 nchunks_out);
    if (rc) return rc;
    // one buffer resource each: the weight planes and the colour sets stay below 2^31 bytes
    if (weights && a->pass.stride * 4 * (int64_t)weight_sets >= ((int64_t)1 << 31)) return PCL_EINVAL;
    if (color_sets > 1 ? pcl_cloud_sets_bytes(n, color_sets) == 0 : a->pass.stride * 6 * 4 >= ((int64_t)1 << 31)) return PCL_EINVAL;
    a->weights = weights;
    im->sets = color_sets > 1 ? color_sets : 1; im->img0 = 0; im->btot = nimages; im->wsets = weights ? weight_sets : 1;
    return 0;
}

// One launch's slice of a call: the run of at most PCL_RES_MAX_IMAGES images from image i0 on.  *al, *il are the call's a, im with the run's
// panorama table, img0 = i0, the poses sliced (pose_stride floats per pose from a.pass.trans / rot) and the launch's pose count.  -> that count
static inline int pcl_info_slice(const PclInfoArgs& a, const PclInfoImages& im, const uint64_t* panos_host, int i0, PclInfoArgs* al, PclInfoImages* il)
{
    const int m = im.btot - i0 < PCL_RES_MAX_IMAGES ? im.btot - i0 : PCL_RES_MAX_IMAGES;
    *il = im;
    for (int i = 0; i < PCL_RES_MAX_IMAGES; i++) il->panos.p[i] = i < m ? (unsigned long long)panos_host[i0 + i] : 0ull;
    il->img0 = i0;
    *al = a;
    al->pass.trans = a.pass.trans + (int64_t)i0 * a.pass.pose_stride; al->pass.rot = a.pass.rot + (int64_t)i0 * a.pass.pose_stride;
    al->pass.B = m;
    return m;
}

// The launches of one evaluation of all the images: launch(al, il, i0, grid) for every such run, the colour set, weight plane and partial
// row counted from the call's first image
template <class F>
static inline void pcl_info_images_launches(const PclInfoArgs& a, const PclInfoImages& im, const uint64_t* panos_host, int64_t nchunks, F&& launch)
{
    for (int i0 = 0; i0 < im.btot; i0 += PCL_RES_MAX_IMAGES) {
        PclInfoArgs al;
        PclInfoImages il;
        const int m = pcl_info_slice(a, im, panos_host, i0, &al, &il);
        launch(al, il, i0, dim3((unsigned)(nchunks * m)));
    }
}

// ---- host side of the rooms entry points (pcl_pose_information_rooms, pcl_gn_refine_rooms): every check, before any launch
struct PclInfoRoomsPlan {
    PclInfoRooms t;              // block0 is filled per launch (pcl_info_rooms_launches)
    int nrooms;
    size_t bytes;                // every room's region [nchunks_r][nimages][PCL_INFO_ROW], each 256-byte aligned: the workspace
};

// The rooms' chunkings and regions (they depend on n_r and nimages alone); PCL_EINVAL: nrooms outside 1..PCL_GD_MAX_ROOMS, nimages < 1, a
// room with a null cloud or n outside 1..PCL_MAX_POINTS, more blocks than a grid holds.  pcl_gd_room.box is not read.
static inline int pcl_info_rooms_plan(const pcl_gd_room* rooms_host, int nrooms, int nimages, PclInfoRoomsPlan* g)
{
    if (!rooms_host || nrooms < 1 || nrooms > PCL_GD_MAX_ROOMS || nimages < 1) return PCL_EINVAL;
    memset(&g->t, 0, sizeof(g->t));
    for (int r = 0; r < PCL_GD_MAX_ROOMS; r++) g->t.block0[r] = 0x7fffffff;
    g->nrooms = nrooms;
    PclCarve c{nullptr, 0};
    int64_t chunks = 0;
    for (int r = 0; r < nrooms; r++) {
        const int64_t n = rooms_host[r].n;
        if (!rooms_host[r].cloud || n <= 0 || n > PCL_MAX_POINTS) return PCL_EINVAL;
        int64_t steps;
        const int64_t nchunks = pcl_pass_chunks(n, PCL_INFO_MIN_STEPS, &steps);
        PclInfoRoom& e = g->t.rec[r];
        e.cloud = (unsigned long long)rooms_host[r].cloud;
        e.n = (int)n; e.stride = (int)pcl_cloud_stride(n);
        e.nchunks = (int)nchunks; e.steps_base = (int)(steps / nchunks); e.steps_rem = (int)(steps % nchunks);
        e.rows = (long long)(c.off / sizeof(float));
        c.take((size_t)nchunks * (size_t)nimages * PCL_INFO_ROW * sizeof(float));
        chunks += nchunks;
    }
    if (chunks * nimages > 0x7fffffffll) return PCL_EINVAL;
    g->bytes = c.off;
    return 0;
}

// Everything the rooms entry points check beside their own outputs, and what their launches share: a (a.pass.B = nimages; the cloud
// fields are room 0's and no kernel reads them), im, the plan.  color_sets 0 / 1, or nimages: every room's cloud has that many sets.
static inline int pcl_info_rooms_args(PclInfoArgs* a, PclInfoImages* im, PclInfoRoomsPlan* g, const pcl_gd_room* rooms_host, int nrooms, int color_sets,
                                      const uint64_t* panos_host, int nimages, int pano_format, int H, int W, const float* trans, const float* rot,
                                      int pose_stride)
{
    if (!panos_host || nimages <= 0) return PCL_EINVAL;
    for (int i = 0; i < nimages; i++)
        if (!panos_host[i]) return PCL_EINVAL;
    if (color_sets < 0 || (color_sets > 1 && color_sets != nimages)) return PCL_EINVAL;
    int rc = pcl_info_rooms_plan(rooms_host, nrooms, nimages, g);
    if (rc) return rc;
    int64_t nchunks0;
    rc = pcl_pass_args(&a->pass, (const float*)rooms_host[0].cloud, rooms_host[0].n, (const void*)panos_host[0], pano_format, H, W, trans, rot, pose_stride,
                       nimages, PCL_INFO_MIN_STEPS, &nchunks0);
    if (rc) return rc;
    // one buffer resource per room: its colour sets stay below 2^31 bytes
    for (int r = 0; r < nrooms; r++)
        if (color_sets > 1 ? pcl_cloud_sets_bytes(rooms_host[r].n, color_sets) == 0 : (int64_t)g->t.rec[r].stride * 6 * 4 >= ((int64_t)1 << 31)) return PCL_EINVAL;
    a->weights = nullptr;
    im->sets = color_sets > 1 ? color_sets : 1; im->img0 = 0; im->btot = nimages; im->wsets = 1;
    return 0;
}

// The launches of one evaluation of all rooms x images: launch(al, il, tl, i0, grid) for every run of pcl_info_slice, all rooms in each,
// the rooms' block ranges laid out for the run's image count
template <class F>
static inline void pcl_info_rooms_launches(const PclInfoArgs& a, const PclInfoImages& im, const PclInfoRoomsPlan& g, const uint64_t* panos_host, F&& launch)
{
    for (int i0 = 0; i0 < im.btot; i0 += PCL_RES_MAX_IMAGES) {
        PclInfoArgs al;
        PclInfoImages il;
        const int m = pcl_info_slice(a, im, panos_host, i0, &al, &il);
        PclInfoRooms tl = g.t;
        int64_t blocks = 0;
        for (int r = 0; r < g.nrooms; r++) {
            tl.rec[r].block0 = tl.block0[r] = (int)blocks;
            blocks += (int64_t)tl.rec[r].nchunks * m;
        }
        launch(al, il, tl, i0, dim3((unsigned)blocks));
    }
}
