// pcl_score.hip — score maps: what the histogram stage's table of patch intersections says about the image patches and about the
// points, averaged over the candidate poses (additive to ABI 12; BUILD-DEFINED, include/piccolo_hip.h states the rules).
//
//   pcl_score_maps      score2d[j] = mean over the poses k with valid(k, j) of inter[k][j], valid(k, j) = nproj[k][j] > 0 && nimg[j] > 0;
//                       score3d[p] = mean over the poses k of inter[k][j(k, p)] where point p's centre pixel lies in scored block j(k, p)
//                       and valid(k, j); -1 and count 0 where nothing voted.  Sums in fp32, poses ascending, one division.
//   pcl_score_weights   a packed weight plane from a 3D map: the voted scores stretched from [lo, hi] to [floor, 1], 1 without evidence
//
// Two launches for the maps.  pcl_score_prepare_kernel writes the poses' records (pcl_write_pose_rec: the histogram stage's R, bit for
// bit), the 2D map, and the validity-folded table tab[K][nblk + 1]: inter where valid, -1 elsewhere, and -1 in the extra column nblk,
// which is where a point in no block looks.  A pose that is not finite has -1 in its whole row.  pcl_score_points_kernel then gives
// every lane PER packed points for the whole call: coordinates and (sum, count) stay in registers, the poses are walked in ascending
// order (that order IS the result's rounding), a pose's record is read through a uniform address, and a vote is one table read, one
// compare and two adds.  No atomics, no scratch, no LDS in the shipped form; nothing is allocated and nobody waits for the host
// (capturable).
// The pixel is pcl_bin_project's: R (x - t) with the same fma chain, then the loss kernel's fast arctangents (pcl_pano_coord_fast).  Only
// BLOCK borders matter here: the fast coordinates are within `margin` of the reference formula's (pcl_pano_pixel_fast's certificate),
// so a point whose fast coordinate is farther than that from every multiple of the block size and from the image's edges is in the
// block of the reference formula's pixel whichever pixel of that block it is.  The others (2 margin / bh of the points, and NaNs) are
// recomputed in place with pcl_pano_pixel_ref.
#include <algorithm>

#include "pcl_host.h"
#include "pcl_pano_pixel.h"

#define PCL_SCORE_MAX_POSES 65535
#define PCL_SCORE_MAX_SIDE 65535        // H, W: the block of a pixel is a float multiply (pcl_score_block)
#define PCL_SCORE_LDS_BYTES 32768       // the pose chunk of the LDS form (experiments build, PCL_SCORE_LDS=1)

struct PclScoreArgs {
    const float* cloud;
    int64_t n, stride;
    const PclPoseRec* recs;
    const float* table;      // [K][nblk + 1]
    const int64_t* order;    // ORDERED: packed slot -> the caller's point index
    float* score3d;
    int32_t* count3d;
    int K, H, W, nsh, nsw, nblk;
    float fbh, fbw, inv_bh, inv_bw;      // block size in pixels and its reciprocal
    float margin_x, margin_y;
    int chunk;               // LDS form: poses per staged chunk
};

// the scored block (h - 1) * nsw + w of a pixel, nblk for a pixel in none.  (row + 0.5) / bh has a fractional part in [0.5 / bh, 1 - 0.5 / bh];
// the product below is off by at most 3 x 2^-24 (row / bh) < 0.5 / bh for H < 2^21: its truncation is row / bh.
__device__ __forceinline__ int pcl_score_block(const PclScoreArgs& a, int row, int col)
{
    const int h = (int)(((float)row + 0.5f) * a.inv_bh), w = (int)(((float)col + 0.5f) * a.inv_bw);
    return (h >= 1 && h <= a.nsh - 2 && w >= 0 && w < a.nsw) ? (h - 1) * a.nsw + w : a.nblk;
}

// the block of packed point (x, y, z) for pose pr — always in [0, nblk]
__device__ __forceinline__ int pcl_score_project(const PclScoreArgs& a, const PclPoseRec* __restrict__ pr, float x, float y, float z)
{
    const float qx = x - pr->t[0], qy = y - pr->t[1], qz = z - pr->t[2];
    const float px = fmaf(pr->R[2], qz, fmaf(pr->R[1], qy, pr->R[0] * qx));
    const float py = fmaf(pr->R[5], qz, fmaf(pr->R[4], qy, pr->R[3] * qx));
    const float pz = fmaf(pr->R[8], qz, fmaf(pr->R[7], qy, pr->R[6] * qx));
    float cx, cy;
    pcl_pano_coord_fast(px, py, pz, a.H, a.W, cx, cy);
    // distance to the nearest multiple of the block size: k * b is exact, the fma rounds once
    const float ky = rintf(cy * a.inv_bh), kx = rintf(cx * a.inv_bw);
    const float dy = fabsf(fmaf(-ky, a.fbh, cy)), dx = fabsf(fmaf(-kx, a.fbw, cx));
    // (a NaN coordinate fails every compare: not certain)
    const bool certain = dy > a.margin_y && dx > a.margin_x && cy > a.margin_y && cy < (float)(a.H - 1) - a.margin_y && cx > a.margin_x &&
                         cx < (float)(a.W - 1) - a.margin_x;
    int row = (int)cy, col = (int)cx;
    if (!certain) pcl_pano_pixel_ref(px, py, pz, a.H, a.W, row, col);
    return pcl_score_block(a, row, col);
}

template <int PER, bool ORDERED, bool LDS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_score_points_kernel(PclScoreArgs a)
{
    extern __shared__ float stab[];                    // LDS form: [chunk][nblk + 1]
    const int64_t first = (int64_t)blockIdx.x * (PCL_BLOCK * PER) + threadIdx.x;
    float x[PER], y[PER], z[PER], sum[PER];
    int cnt[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int64_t i = first + (int64_t)u * PCL_BLOCK;
        const bool live = i < a.n;                     // (a lane without a point walks the origin: its block index is in range, nothing is stored)
        x[u] = live ? a.cloud[i] : 0.f;
        y[u] = live ? a.cloud[a.stride + i] : 0.f;
        z[u] = live ? a.cloud[2 * a.stride + i] : 0.f;
        sum[u] = 0.f; cnt[u] = 0;
    }
    const int width = a.nblk + 1;
    if constexpr (LDS) {
        for (int k0 = 0; k0 < a.K; k0 += a.chunk) {
            const int kn = min(a.chunk, a.K - k0);
            __syncthreads();                           // the previous chunk has been read
            for (int i = threadIdx.x; i < kn * width; i += PCL_BLOCK) stab[i] = a.table[(int64_t)k0 * width + i];
            __syncthreads();
            for (int k = 0; k < kn; k++) {
                const PclPoseRec* __restrict__ pr = a.recs + (k0 + k);
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const float v = stab[k * width + pcl_score_project(a, pr, x[u], y[u], z[u])];
                    if (v >= 0.f) { sum[u] += v; cnt[u] += 1; }
                }
            }
        }
    } else {
        for (int k = 0; k < a.K; k++) {
            const PclPoseRec* __restrict__ pr = a.recs + k;
            const float* __restrict__ row = a.table + (int64_t)k * width;
#pragma unroll
            for (int u = 0; u < PER; u++) {
                const float v = row[pcl_score_project(a, pr, x[u], y[u], z[u])];
                if (v >= 0.f) { sum[u] += v; cnt[u] += 1; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int64_t i = first + (int64_t)u * PCL_BLOCK;
        if (i >= a.n) continue;
        int64_t o = i;
        if constexpr (ORDERED) {
            o = a.order[i];
            if ((uint64_t)o >= (uint64_t)a.n) continue;
        }
        a.score3d[o] = cnt[u] ? __fdiv_rn(sum[u], (float)cnt[u]) : -1.f;
        a.count3d[o] = cnt[u];
    }
}

// Everything before the points: the poses' records, the validity-folded table and the 2D map, in one launch.  Grid-stride sections;
// every word is written by exactly one thread.  table / recs null: only the 2D map; score2d null: only the table.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_score_prepare_kernel(const float* __restrict__ trans, const float* __restrict__ rot, int K, int nblk,
                                                                      const float* __restrict__ inter, const int* __restrict__ nproj,
                                                                      const int* __restrict__ nimg, PclPoseRec* __restrict__ recs,
                                                                      float* __restrict__ table, float* __restrict__ score2d, int32_t* __restrict__ count2d)
{
    const int64_t tid = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x, nth = (int64_t)gridDim.x * PCL_BLOCK;
    if (table) {
        if (tid < K) {
            const int b = (int)tid;
            float p[6] = {trans[3 * b], trans[3 * b + 1], trans[3 * b + 2], rot[3 * b], rot[3 * b + 1], rot[3 * b + 2]};
            pcl_write_pose_rec(&recs[b], p);
        }
        const int width = nblk + 1;
        for (int64_t i = tid; i < (int64_t)K * width; i += nth) {
            const int k = (int)(i / width), j = (int)(i - (int64_t)k * width);
            float v = -1.f;
            if (j < nblk) {
                bool finite = true;                    // a pose that is not finite casts no vote
                for (int c = 0; c < 3; c++) finite = finite && fabsf(trans[3 * k + c]) <= 3.402823466e38f && fabsf(rot[3 * k + c]) <= 3.402823466e38f;
                if (finite && nproj[(int64_t)k * nblk + j] > 0 && nimg[j] > 0) v = inter[(int64_t)k * nblk + j];
            }
            table[i] = v;
        }
    }
    if (score2d)
        for (int64_t j = tid; j < nblk; j += nth) {
            float s = 0.f;
            int c = 0;
            if (nimg[j] > 0)
                for (int k = 0; k < K; k++)
                    if (nproj[(int64_t)k * nblk + j] > 0) { s += inter[(int64_t)k * nblk + j]; c += 1; }
            score2d[j] = c ? __fdiv_rn(s, (float)c) : -1.f;
            count2d[j] = c;
        }
}

struct PclScoreWs { PclPoseRec* recs; float* table; };
static size_t score_layout(void* base, int K, int nsh, int nsw, PclScoreWs* w)
{
    PclCarve c{(char*)base, 0};
    w->recs = (PclPoseRec*)c.take((size_t)K * sizeof(PclPoseRec));
    w->table = (float*)c.take((size_t)K * ((size_t)(nsh - 2) * nsw + 1) * sizeof(float));
    return c.off;
}

static bool score_shape_ok(int64_t n, int K, int nsh, int nsw)
{
    return n > 0 && n <= PCL_MAX_POINTS && K >= 1 && K <= PCL_SCORE_MAX_POSES && nsh >= 3 && nsh <= PCL_SCORE_MAX_SIDE && nsw >= 1 &&
           nsw <= PCL_SCORE_MAX_SIDE && (int64_t)(nsh - 2) * nsw < ((int64_t)1 << 24);
}

extern "C" size_t pcl_score_maps_workspace_bytes(int64_t n, int K, int nsh, int nsw)
{
    PclScoreWs w;
    return score_shape_ok(n, K, nsh, nsw) ? score_layout(nullptr, K, nsh, nsw, &w) : 0;
}

extern "C" int pcl_score_maps(const float* cloud, int64_t n, const float* trans, const float* rot, int K, int H, int W, int nsh, int nsw,
                              const float* inter, const int32_t* nproj, const int32_t* nimg, const int64_t* order, float* score3d, int32_t* count3d,
                              float* score2d, int32_t* count2d, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!cloud || !trans || !rot || !inter || !nproj || !nimg || !workspace) return PCL_EINVAL;
    if ((score3d == nullptr) != (count3d == nullptr) || (score2d == nullptr) != (count2d == nullptr) || (!score3d && !score2d)) return PCL_EINVAL;
    if (!score_shape_ok(n, K, nsh, nsw) || H <= 0 || W <= 0 || H > PCL_SCORE_MAX_SIDE || W > PCL_SCORE_MAX_SIDE) return PCL_EINVAL;
    const int bh = H / nsh, bw = W / nsw, nblk = (nsh - 2) * nsw;
    if (bh <= 0 || bw <= 0) return PCL_EINVAL;
    PclScoreWs w;
    if (workspace_bytes < score_layout(workspace, K, nsh, nsw, &w)) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    {
        const int64_t work = std::max((int64_t)nblk, score3d ? (int64_t)K * (nblk + 1) : (int64_t)0);
        const int64_t blocks = (work + PCL_BLOCK - 1) / PCL_BLOCK;
        hipLaunchKernelGGL(pcl_score_prepare_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(PCL_BLOCK), 0, s, trans, rot, K, nblk, inter,
                           nproj, nimg, w.recs, score3d ? w.table : (float*)nullptr, score2d, count2d);
    }
    if (score3d) {
        PclScoreArgs a;
        a.cloud = cloud; a.n = n; a.stride = pcl_cloud_stride(n); a.recs = w.recs; a.table = w.table; a.order = order;
        a.score3d = score3d; a.count3d = count3d;
        a.K = K; a.H = H; a.W = W; a.nsh = nsh; a.nsw = nsw; a.nblk = nblk;
        a.fbh = (float)bh; a.fbw = (float)bw; a.inv_bh = 1.0f / (float)bh; a.inv_bw = 1.0f / (float)bw;
        // pcl_pano_pixel_fast's certificate, as the histogram stage sets it: 1.5e-6 x the image size, at least 1e-3 pixel
        a.margin_x = fmaxf(1e-3f, 1.5e-6f * (float)W); a.margin_y = fmaxf(1e-3f, 1.5e-6f * (float)H);
        // Table placement: the L2-resident global table ships; the experiments build stages chunks of poses in LDS on
        // request (PCL_SCORE_LDS=1, tools/score_map_bench.py), where a pose's row fits
        const size_t row_bytes = (size_t)(nblk + 1) * sizeof(float);
        const bool lds = PCL_KNOB(SCORE_LDS, 0) != 0 && row_bytes <= PCL_SCORE_LDS_BYTES;
        a.chunk = lds ? (int)std::min<size_t>(PCL_SCORE_LDS_BYTES / row_bytes, (size_t)K) : 0;
        // two points per lane once that still fills the chip (256 CUs x 8 blocks); one below
        const bool two = n >= (int64_t)1 << 20;
        pcl_with_flag(two, [&](auto t2) {
            constexpr int PER = decltype(t2)::value ? 2 : 1;
            const dim3 grid((unsigned)((n + PCL_BLOCK * PER - 1) / (PCL_BLOCK * PER))), blk(PCL_BLOCK);
            pcl_with_flag(order != nullptr, [&](auto ord) {
#ifdef PCL_EXPERIMENTS
                if (lds) {
                    hipLaunchKernelGGL((pcl_score_points_kernel<PER, decltype(ord)::value, true>), grid, blk, (size_t)a.chunk * row_bytes, s, a);
                    return;
                }
#endif
                hipLaunchKernelGGL((pcl_score_points_kernel<PER, decltype(ord)::value, false>), grid, blk, 0, s, a);
            });
        });
    }
    PCL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// weight plane from a 3D map: lo / hi = the smallest / largest score over the points with at least min_count votes, by integer atomic
// min / max on the bit patterns (the scores are >= 0: ascending floats are ascending integers, and the result does not depend on
// scheduling); then w = fma(1 - floor, (s - lo) / (hi - lo), floor) clamped to [0, 1], one rounding per operation.

struct PclScoreRange { uint32_t lo, hi, voted, pad; };

__global__ void pcl_score_range_init_kernel(PclScoreRange* st)
{
    st->lo = 0xffffffffu; st->hi = 0u; st->voted = 0u; st->pad = 0u;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_score_range_kernel(const float* __restrict__ score, const int32_t* __restrict__ count, int64_t n,
                                                                    int min_count, PclScoreRange* st)
{
    __shared__ uint32_t red[3];
    if (threadIdx.x == 0) { red[0] = 0xffffffffu; red[1] = 0u; red[2] = 0u; }
    __syncthreads();
    uint32_t lo = 0xffffffffu, hi = 0u, voted = 0u;
    for (int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PCL_BLOCK) {
        if (count[i] < min_count) continue;
        const uint32_t u = __float_as_uint(score[i]);
        lo = min(lo, u); hi = max(hi, u); voted += 1u;
    }
    if (voted) { atomicMin(&red[0], lo); atomicMax(&red[1], hi); atomicAdd(&red[2], voted); }
    __syncthreads();
    if (threadIdx.x == 0 && red[2]) { atomicMin(&st->lo, red[0]); atomicMax(&st->hi, red[1]); atomicAdd(&st->voted, red[2]); }
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_score_plane_kernel(const float* __restrict__ score, const int32_t* __restrict__ count, int64_t n,
                                                                    int64_t stride, int min_count, float floor_w, const PclScoreRange* __restrict__ st,
                                                                    float* __restrict__ plane, float* __restrict__ range_out)
{
    const uint32_t voted = st->voted;
    const float lo = voted ? __uint_as_float(st->lo) : 0.f, hi = voted ? __uint_as_float(st->hi) : 0.f;
    if (range_out && blockIdx.x == 0 && threadIdx.x == 0) { range_out[0] = lo; range_out[1] = hi; range_out[2] = (float)voted; }
    const bool flat = voted == 0u || hi == lo;         // no evidence, or none that tells two points apart: every point weighs 1
    const float span = __fsub_rn(hi, lo), gain = __fsub_rn(1.0f, floor_w);
    for (int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x; i < stride; i += (int64_t)gridDim.x * PCL_BLOCK) {
        float w = 0.f;                                 // padding
        if (i < n) {
            w = 1.f;
            if (!flat && count[i] >= min_count) {
                w = fmaf(gain, __fdiv_rn(__fsub_rn(score[i], lo), span), floor_w);
                w = fminf(fmaxf(w, 0.f), 1.f);
            }
        }
        plane[i] = w;
    }
}

static size_t score_weights_layout(void* base, PclScoreRange** st)
{
    PclCarve c{(char*)base, 0};
    *st = (PclScoreRange*)c.take(sizeof(PclScoreRange));
    return c.off;
}

extern "C" size_t pcl_score_weights_workspace_bytes(int64_t n)
{
    PclScoreRange* st;
    return n <= 0 || n > PCL_MAX_POINTS ? 0 : score_weights_layout(nullptr, &st);
}

extern "C" int pcl_score_weights(const float* score_packed, const int32_t* count_packed, int64_t n, int min_count, float floor, float* plane,
                                 float* range_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!score_packed || !count_packed || !plane || !workspace || n <= 0 || n > PCL_MAX_POINTS || min_count < 1) return PCL_EINVAL;
    if (!(floor >= 0.f && floor < 1.f)) return PCL_EINVAL;
    PclScoreRange* st;
    if (workspace_bytes < score_weights_layout(workspace, &st)) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = pcl_cloud_stride(n), want = stride / PCL_BLOCK;
    const dim3 grid((unsigned)(want < 1024 ? want : 1024)), blk(PCL_BLOCK);
    hipLaunchKernelGGL(pcl_score_range_init_kernel, dim3(1), dim3(1), 0, s, st);
    hipLaunchKernelGGL(pcl_score_range_kernel, grid, blk, 0, s, score_packed, count_packed, n, min_count, st);
    hipLaunchKernelGGL(pcl_score_plane_kernel, grid, blk, 0, s, score_packed, count_packed, n, stride, min_count, floor, st, plane, range_out);
    PCL_LAUNCH_CHECK();
    return 0;
}
