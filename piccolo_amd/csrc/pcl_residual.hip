// pcl_residual.hip — what the loss kernel sums, per point, and a robust weight plane made from it on the device (additive to ABI 12).
//
//   pcl_point_residuals   residual[b][i] = ||c_bi - rgb_i|| where the loss kernel's mask keeps point i at pose b, exactly -1 where the sampled
//                         colour is exactly (0, 0, 0), NaN at a pose that is not finite — one forward-only launch beside the loss kernel,
//                         whose instances are left as they are
//   pcl_robust_weights    s = lower median of one residual row's unmasked entries (exact MSB radix select over the bit patterns, integer
//                         atomics only), c = k s, and the truncated / Huber weight of every point into a packed weight plane
//   pcl_point_residuals_images / pcl_robust_weights_rows   the same for the I winners of a chain of I query images in the same launches: row i
//                         against panorama i (and colour set i), plane i from row i — what pcl_gd_run_weight_sets' planes are made from
//
// Both residual kernels are the per-point pass of pcl_point_pass.h (built from the device functions the loss kernel is built from: the
// weighted forward-only instance of pcl_sample2 with unit weights and fresh accumulators) with ONE body for what becomes of a pair: a lane
// ends with exactly the two numbers the loss kernel would have added for its two points, acc[0] = n2 * rsq(n2 + 1e-37) under the mask and
// acc[1] = the mask bit, and stores them.  Same instructions on the same inputs: the kept set is the loss kernel's count, bit for bit, and
// the kept values differ from its sum by the summation order only.
// Mapping: 256-thread blocks, a lane carries the two ADJACENT packed slots 2 t, 2 t + 1 of a 512-slot step (the loss kernel pairs slot t
// with t + 256: the packed halves never interact, so the pairing changes no value), which makes the cloud six 8-byte loads per lane and the
// packed-order output one 8-byte store.  No LDS, no atomics, no scratch; no allocation and no synchronisation on the host side
// (capturable).  The grid is chunks x poses with the pose varying fastest (blocks resident together read the same chunk); it need not be
// pcl_plan's, because nothing is summed.  The two entry points differ in their launch shape only: any B poses on one panorama in one
// launch, against up to PCL_RES_MAX_IMAGES panorama addresses as kernel arguments.
// The robust weights have ONE rows path: the row is blockIdx.y, and a single row is the rows form with one row.
#include "pcl_point_pass.h"

struct PclResArgs {
    PclPassArgs pass;
    const int64_t* order;    // ORDERED: packed slot -> the caller's point index
    float* residual;         // [B][n]
};

typedef float pcl_f2u __attribute__((ext_vector_type(2), aligned(4)));      // a row of n floats starts on a 4-byte boundary only

// row b of the residuals from pose b against `pano_b` (and, with CS, colour set `set` of `sets`)
template <int FMT, bool ORDERED, bool CS>
__device__ __forceinline__ void pcl_res_body(const PclResArgs& a, const void* pano_b, int sets, unsigned set)
{
    const int64_t n = a.pass.n;
    float* __restrict__ row = a.residual + (int64_t)(blockIdx.x % (unsigned)a.pass.B) * n;
    pcl_point_pass<FMT, false, CS>(a.pass, pano_b, sets, set, [&](int i0, int, bool valid0, bool valid1, const f2* acc, bool pose_ok) {
        const float r0 = pcl_res_value(acc[0].x, acc[1].x, pose_ok), r1 = pcl_res_value(acc[0].y, acc[1].y, pose_ok);
        if constexpr (ORDERED) {
            if (valid0) {
                const int64_t o = a.order[i0];
                if ((uint64_t)o < (uint64_t)n) row[o] = r0;
            }
            if (valid1) {
                const int64_t o = a.order[i0 + 1];
                if ((uint64_t)o < (uint64_t)n) row[o] = r1;
            }
        } else {
            if (valid1) *reinterpret_cast<pcl_f2u*>(row + i0) = (pcl_f2u){r0, r1};
            else if (valid0) row[i0] = r0;
        }
    });
}

template <int FMT, bool ORDERED>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_point_residuals_kernel(PclResArgs a)
{
    pcl_res_body<FMT, ORDERED, false>(a, a.pass.pano, 1, 0);
}

// Row i = pose i against panorama i (and colour set i): the panorama addresses travel as kernel arguments, up to PCL_RES_MAX_IMAGES per
// launch (PclResPanos, pcl_point_pass.h); `img0` is the first image of this launch (the colour set counts from the call's first image,
// a.pass.B is this launch's pose count)
template <int FMT, bool ORDERED, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_point_residuals_images_kernel(PclResArgs a, PclResPanos panos, int sets, int img0)
{
    const unsigned b = blockIdx.x % (unsigned)a.pass.B;
    pcl_res_body<FMT, ORDERED, CS>(a, (const void*)panos.p[b], sets, b + (unsigned)img0);                  // (b: from the block index, uniform)
}

// what both entry points check and fill; the grid is nchunks x B
static int res_args(PclResArgs* a, const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans, const float* rot,
                    int pose_stride, int B, const int64_t* order, float* residual, int64_t* nchunks_out)
{
    if (!residual) return PCL_EINVAL;
    a->order = order; a->residual = residual;
    return pcl_pass_args(&a->pass, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, 1, nchunks_out);
}

extern "C" int pcl_point_residuals(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans, const float* rot,
                                   int pose_stride, int B, const int64_t* order, float* residual, void* stream)
{
    PclResArgs a;
    int64_t nchunks;
    const int rc = res_args(&a, cloud, n, pano, pano_format, H, W, trans, rot, pose_stride, B, order, residual, &nchunks);
    if (rc) return rc;
    const dim3 grid((unsigned)(nchunks * B)), blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    pcl_with_flag(order != nullptr, [&](auto ord) {
        pcl_with_pass_fmt(pano_format, [&](auto fmt) {
            hipLaunchKernelGGL((pcl_point_residuals_kernel<decltype(fmt)::value, decltype(ord)::value>), grid, blk, 0, s, a);
        });
    });
    PCL_LAUNCH_CHECK();
    return 0;
}

// Row i = pcl_point_residuals of pose i against panos_host[i] and, with color_sets == nimages, colour set i of a cloud of pcl_cloud_pack_sets:
// the same body, so the same bits.  One launch per PCL_RES_MAX_IMAGES images; the addresses are kernel arguments (capturable, no copy).
extern "C" int pcl_point_residuals_images(const float* cloud, int64_t n, int color_sets, const uint64_t* panos_host, int nimages, int pano_format, int H,
                                          int W, const float* trans, const float* rot, int pose_stride, const int64_t* order, float* residual,
                                          void* stream)
{
    if (!panos_host || nimages <= 0 || color_sets < 0 || (color_sets > 1 && color_sets != nimages)) return PCL_EINVAL;
    for (int i = 0; i < nimages; i++)
        if (!panos_host[i]) return PCL_EINVAL;
    PclResArgs a;
    int64_t nchunks;
    int rc = res_args(&a, cloud, n, (const void*)panos_host[0], pano_format, H, W, trans, rot, pose_stride, nimages, order, residual, &nchunks);
    if (rc) return rc;
    const bool sets = color_sets > 1;
    if (sets && pcl_cloud_sets_bytes(n, color_sets) == 0) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    for (int i0 = 0; i0 < nimages; i0 += PCL_RES_MAX_IMAGES) {
        const int m = nimages - i0 < PCL_RES_MAX_IMAGES ? nimages - i0 : PCL_RES_MAX_IMAGES;
        PclResPanos list;
        for (int i = 0; i < PCL_RES_MAX_IMAGES; i++) list.p[i] = i < m ? (unsigned long long)panos_host[i0 + i] : 0ull;
        PclResArgs al = a;
        al.pass.trans = trans + (int64_t)i0 * pose_stride; al.pass.rot = rot + (int64_t)i0 * pose_stride;
        al.residual = residual + (int64_t)i0 * n; al.pass.B = m;
        const dim3 grid((unsigned)(nchunks * m)), blk(PCL_BLOCK);
        pcl_with_flag(order != nullptr, [&](auto ord) {
            pcl_with_flag(sets, [&](auto cs) {
                pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                    hipLaunchKernelGGL((pcl_point_residuals_images_kernel<decltype(fmt)::value, decltype(ord)::value, decltype(cs)::value>), grid, blk, 0,
                                       s, al, list, color_sets, i0);
                });
            });
        });
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// robust weights: the scale of every residual row and its weight plane, pcl_quantile_box's way — an exact order statistic by a 4-pass MSB
// radix select over order-preserving uint32 keys, integer atomics only, so the result does not depend on scheduling.  The rank is not
// known beforehand (M, the number of entries that are not -1, is pass 0's total), and there is no scan launch: every block of a later
// pass resolves the earlier passes' histograms itself (256 counts each), and so does the weight kernel.  Six launches in all, for any
// number of rows: the row is blockIdx.y — its residuals n floats, its histograms one PclRobustState, its plane `stride` floats and its
// (s, M) two floats behind the previous row's.  The counts are integers, so a row's plane and scale do not depend on the rows beside it.

struct PclRobustState { uint32_t hist[4][256]; };                  // (n <= 2^27: a count fits 32 bits)
struct PclRobustWs { PclRobustState* st; };                        // one state per row, back to back
static size_t robust_layout(void* base, int nrows, PclRobustWs* w)
{
    PclCarve c{(char*)base, 0};
    w->st = (PclRobustState*)c.take((size_t)nrows * sizeof(PclRobustState));
    return c.off;
}

extern "C" size_t pcl_robust_weights_workspace_bytes(int64_t n)
{
    PclRobustWs w;
    return n <= 0 || n > PCL_MAX_POINTS ? 0 : robust_layout(nullptr, 1, &w);
}

#define PCL_ROBUST_MAX_ROWS 65535                                  // (the row is the grid's second dimension)
extern "C" size_t pcl_robust_weights_rows_workspace_bytes(int64_t n, int nrows)
{
    PclRobustWs w;
    return n <= 0 || n > PCL_MAX_POINTS || nrows < 1 || nrows > PCL_ROBUST_MAX_ROWS ? 0 : robust_layout(nullptr, nrows, &w);
}

// ascending floats -> ascending keys; every NaN is ONE key behind +inf (a NaN residual comes from a NaN pose, with either sign bit)
__device__ __forceinline__ uint32_t pcl_rw_key(float l)
{
    uint32_t u = l != l ? 0x7fc00000u : __float_as_uint(l);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pcl_rw_key2f(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// What the first `npass` histograms say, computed by all 256 threads of a block: M, the known high bytes of the wanted key and the wanted
// rank among the entries that share them.  The wanted rank is (M - 1) / 2, the lower median.
__device__ __forceinline__ void pcl_rw_resolve(const PclRobustState* st, int npass, uint32_t& prefix, uint32_t& rank, uint32_t& M)
{
    __shared__ uint32_t wave_tot[PCL_BLOCK / PCL_WAVE], sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    prefix = 0u; rank = 0u; M = 0u;
    for (int p = 0; p < npass; p++) {
        const uint32_t h = st->hist[p][tid];
        uint32_t incl = h;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        if (tid == 0) { sel[0] = 0u; sel[1] = 0u; }
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (int w = 0; w < PCL_BLOCK / PCL_WAVE; w++) {
            if (w < wave) before += wave_tot[w];
            total += wave_tot[w];
        }
        incl += before;
        const uint32_t excl = incl - h;
        if (p == 0) { M = total; rank = M ? (M - 1u) / 2u : 0u; }
        if (excl <= rank && rank < incl) { sel[0] = (uint32_t)tid; sel[1] = excl; }       // exactly one bin (none when M == 0)
        __syncthreads();
        prefix |= sel[0] << (24 - 8 * p);
        rank -= sel[1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_rw_init_kernel(PclRobustState* st)
{
    (&st[blockIdx.y].hist[0][0])[blockIdx.x * PCL_BLOCK + threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_rw_hist_kernel(const float* __restrict__ res, int64_t n, PclRobustState* st, int pass)
{
    res += (int64_t)blockIdx.y * n; st += blockIdx.y;
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    uint32_t prefix, rank, M;
    pcl_rw_resolve(st, pass, prefix, rank, M);
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t known = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PCL_BLOCK) {
        const float l = res[i];
        if (l == -1.0f) continue;                                  // masked at this pose: no evidence
        const uint32_t k = pcl_rw_key(l);
        if ((k & known) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);
}

template <int KIND>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_rw_plane_kernel(const float* __restrict__ res, int64_t n, int64_t stride, const PclRobustState* st, float k,
                                                                 float* __restrict__ plane, float* __restrict__ scale_out)
{
    res += (int64_t)blockIdx.y * n; st += blockIdx.y; plane += (int64_t)blockIdx.y * stride;
    uint32_t prefix, rank, M;
    pcl_rw_resolve(st, 4, prefix, rank, M);
    const float s = M ? pcl_rw_key2f(prefix) : 0.f;
    const float c = __fmul_rn(k, s);
    if (scale_out && blockIdx.x == 0 && threadIdx.x == 0) { scale_out[2 * blockIdx.y] = s; scale_out[2 * blockIdx.y + 1] = (float)M; }
    for (int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x; i < stride; i += (int64_t)gridDim.x * PCL_BLOCK) {
        float w = 0.f;                                             // padding
        if (i < n) {
            const float l = res[i];
            if (l == -1.0f || M == 0u) w = 1.f;
            else if (!(fabsf(l) <= 3.402823466e38f)) w = 0.f;      // NaN or infinite
            else if (l <= c) w = 1.f;
            else if (KIND == PCL_ROBUST_HUBER && c == c) w = __fdiv_rn(c, l);      // (a NaN scale — most of the row NaN — votes 0)
        }
        plane[i] = w;
    }
}

// the checks and the six launches of both entry points
static int robust_rows(const float* residual_packed, int64_t n, int nrows, int kind, float k, float* planes, float* scale_out, void* workspace,
                       size_t workspace_bytes, void* stream)
{
    if (!residual_packed || !planes || !workspace || n <= 0 || n > PCL_MAX_POINTS || nrows < 1 || nrows > PCL_ROBUST_MAX_ROWS) return PCL_EINVAL;
    if ((kind != PCL_ROBUST_TRUNC && kind != PCL_ROBUST_HUBER) || !(k > 0.f && k <= 3.402823466e38f)) return PCL_EINVAL;
    PclRobustWs w;
    if (workspace_bytes < robust_layout(workspace, nrows, &w)) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = pcl_cloud_stride(n), want = stride / PCL_BLOCK;
    const unsigned nblk = (unsigned)(want < 1024 ? want : 1024);
    const dim3 grid(nblk, (unsigned)nrows), blk(PCL_BLOCK);
    hipLaunchKernelGGL(pcl_rw_init_kernel, dim3(4, (unsigned)nrows), blk, 0, s, w.st);
    for (int pass = 0; pass < 4; pass++) hipLaunchKernelGGL(pcl_rw_hist_kernel, grid, blk, 0, s, residual_packed, n, w.st, pass);
    if (kind == PCL_ROBUST_HUBER)
        hipLaunchKernelGGL(pcl_rw_plane_kernel<PCL_ROBUST_HUBER>, grid, blk, 0, s, residual_packed, n, stride, w.st, k, planes, scale_out);
    else
        hipLaunchKernelGGL(pcl_rw_plane_kernel<PCL_ROBUST_TRUNC>, grid, blk, 0, s, residual_packed, n, stride, w.st, k, planes, scale_out);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_robust_weights(const float* residual_packed, int64_t n, int kind, float k, float* plane, float* scale_out, void* workspace,
                                  size_t workspace_bytes, void* stream)
{
    return robust_rows(residual_packed, n, 1, kind, k, plane, scale_out, workspace, workspace_bytes, stream);
}

extern "C" int pcl_robust_weights_rows(const float* residual_packed, int64_t n, int nrows, int kind, float k, float* planes, float* scale_out,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    return robust_rows(residual_packed, n, nrows, kind, k, planes, scale_out, workspace, workspace_bytes, stream);
}
