// pcl_voxel.hip — a voxel grid over a cloud, on the device (additive to ABI 12; build-defined, include/piccolo_hip.h): the voxel of every
// point, the voxels' counts and first points, their centroids, and density weights.  DESIGN.md section 2c.
//
//   pcl_voxel_grid        cell per axis = floor((double)x / voxel) in [-2^20, 2^20) -> a 63-bit key (21 bits per axis) per point; a STABLE
//                         radix sort of (key, point index) pairs puts every voxel's points into one run whose first entry is the voxel's
//                         lowest point index; the runs' first points, flagged in point order and summed by an exclusive scan, number the
//                         voxels in first-occurrence order.  No atomics and no loop whose length depends on the data: the one-voxel cloud and
//                         the cloud of n voxels cost the same.
//   pcl_voxel_centroids   S[v] = sum of llrint(a 65536) over the voxel's points, exact int64, then (float)(S / (count 65536)).  The sums are
//                         integers: any order of summation gives the same bits.  A wave first adds the values of NEIGHBOURING lanes with the
//                         same voxel (a scan in scan order is mostly such runs) and only the last lane of a run goes to memory, so one
//                         destination sees one atomic per wave instead of one per point; the wave's sums then go out transposed,
//                         neighbouring lanes on neighbouring words of a voxel's row.
//   pcl_density_weights   w_i = 1 where count[cell_i] <= cap, else (float)((double)cap / count[cell_i]).
#include "pcl_host.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#define PCL_VOXEL_HALF 1048576            // cells per axis lie in [-2^20, 2^20)
#define PCL_VOXEL_BAD_NONFINITE 1
#define PCL_VOXEL_BAD_CELL 2
#define PCL_VOXEL_BAD_MAGNITUDE 4

// one value of the bad set for a coordinate or colour: 0, or the bits of what is wrong with it
__device__ __forceinline__ int pcl_voxel_value_bad(float a)
{
    if (!(fabsf(a) <= 3.402823466e38f)) return PCL_VOXEL_BAD_NONFINITE;
    return fabsf(a) >= 32768.f ? PCL_VOXEL_BAD_MAGNITUDE : 0;
}

// ---------------------------------------------------------------------------------------------------------------- the grid
__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_key_kernel(const float* __restrict__ xyz, int n, double voxel,
                                                                  unsigned long long* __restrict__ keys, int32_t* __restrict__ iota,
                                                                  int32_t* __restrict__ bad)
{
    const int i = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= n) return;
    unsigned long long key = 0ull;
    int flags = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a = xyz[3 * (int64_t)i + c];
        const int f = pcl_voxel_value_bad(a);
        flags |= f;
        double cell = floor((double)a / voxel);
        if (!(cell >= -(double)PCL_VOXEL_HALF && cell < (double)PCL_VOXEL_HALF)) {          // (NaN fails both)
            if (!(f & PCL_VOXEL_BAD_NONFINITE)) flags |= PCL_VOXEL_BAD_CELL;                // (a finite value: the voxel is too small for it)
            cell = 0.0;                                                                     // a valid key; the caller refuses the result
        }
        key = key << 21 | (unsigned long long)((long long)cell + PCL_VOXEL_HALF);
    }
    keys[i] = key;
    iota[i] = i;
    if (flags) atomicOr(bad, flags);
}

// sorted position j: the position its run starts at where it starts one (else 0, for the running maximum), and a flag on the run's first POINT
__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_heads_kernel(const unsigned long long* __restrict__ keys_sorted,
                                                                   const int32_t* __restrict__ idx_sorted, int n, int32_t* __restrict__ head_raw,
                                                                   int32_t* __restrict__ flag)
{
    const int j = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool head = j == 0 || keys_sorted[j] != keys_sorted[j - 1];
    head_raw[j] = head ? j : 0;
    if (head) flag[idx_sorted[j]] = 1;
}

// head[j]: where j's run starts; its point idx_sorted[head[j]] is the voxel's first, and id[that point] (the exclusive sum of the flags) its
// number.  Every position names its point's voxel; a run's first position writes first[], its last one count[]; position 0 the voxel count.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_finish_kernel(const unsigned long long* __restrict__ keys_sorted,
                                                                    const int32_t* __restrict__ idx_sorted, const int32_t* __restrict__ head,
                                                                    const int32_t* __restrict__ id, const int32_t* __restrict__ flag, int n,
                                                                    int32_t* __restrict__ cell, int32_t* __restrict__ count,
                                                                    int64_t* __restrict__ first, int32_t* __restrict__ nvoxels)
{
    const int j = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int h = head[j];
    const int p = idx_sorted[h];
    const int v = id[p];
    cell[idx_sorted[j]] = v;
    if (h == j) first[v] = p;
    if (j == n - 1 || keys_sorted[j + 1] != keys_sorted[j]) count[v] = j - h + 1;
    if (j == 0) *nvoxels = id[n - 1] + flag[n - 1];
}

static size_t voxel_sort_temp_bytes(int64_t n)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs<rocprim::default_config, const unsigned long long*, unsigned long long*, const int32_t*, int32_t*>(
        nullptr, bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, 63, nullptr, false);
    return bytes;
}

static size_t voxel_scan_temp_bytes(int64_t n)
{
    size_t a = 0, b = 0;
    (void)rocprim::inclusive_scan<rocprim::default_config, const int32_t*, int32_t*, rocprim::maximum<int32_t>>(
        nullptr, a, nullptr, nullptr, (size_t)n, rocprim::maximum<int32_t>(), nullptr, false);
    (void)rocprim::exclusive_scan<rocprim::default_config, const int32_t*, int32_t*, int32_t, rocprim::plus<int32_t>>(
        nullptr, b, nullptr, nullptr, 0, (size_t)n, rocprim::plus<int32_t>(), nullptr, false);
    return a > b ? a : b;
}

// The workspace, carved once for both calls.  The grid: keys, sorted keys, point indices and sorted point indices, the flags, the library's
// temporary storage; after the sort the keys' region holds the scanned run starts and voxel numbers, the indices' region the raw run
// starts.  The centroids: six int64 sums per voxel (at most n voxels) over the same bytes.
struct VoxelWs {
    unsigned long long *keys, *keys_sorted;
    int32_t *iota, *idx_sorted, *flag;
    void* temp;
    size_t temp_bytes;
    long long* sums;
};
static size_t voxel_layout(void* base, int64_t n, VoxelWs* w)
{
    if (n <= 0 || n > PCL_MAX_POINTS) return 0;
    PclCarve c{(char*)base, 0};
    w->keys = (unsigned long long*)c.take((size_t)n * 8);
    w->keys_sorted = (unsigned long long*)c.take((size_t)n * 8);
    w->iota = (int32_t*)c.take((size_t)n * 4);
    w->idx_sorted = (int32_t*)c.take((size_t)n * 4);
    w->flag = (int32_t*)c.take((size_t)n * 4);
    const size_t sort_bytes = voxel_sort_temp_bytes(n), scan_bytes = voxel_scan_temp_bytes(n);
    w->temp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    w->temp = c.take(w->temp_bytes);
    w->sums = (long long*)w->keys;
    const size_t sums_bytes = pcl_align256((size_t)n * 6 * 8);
    return c.off > sums_bytes ? c.off : sums_bytes;
}

extern "C" size_t pcl_voxel_workspace_bytes(int64_t n) { VoxelWs w; return voxel_layout(nullptr, n, &w); }

extern "C" int pcl_voxel_grid(const float* xyz, int64_t n, double voxel, int32_t* cell, int32_t* count, int64_t* first, int32_t* nvoxels,
                              int32_t* bad, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!xyz || !cell || !count || !first || !nvoxels || !bad || !workspace || n <= 0 || n > PCL_MAX_POINTS) return PCL_EINVAL;
    if (!(voxel > 0.0 && voxel <= 1.7976931348623157e308)) return PCL_EINVAL;
    VoxelWs w;
    if (workspace_bytes < voxel_layout(workspace, n, &w)) return PCL_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int m = (int)n;
    const dim3 grid((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), block(PCL_BLOCK);
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.flag, 0, (size_t)n * 4, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_voxel_key_kernel, grid, block, 0, s, xyz, m, voxel, w.keys, w.iota, bad);
    PCL_LAUNCH_CHECK();
    e = rocprim::radix_sort_pairs(w.temp, w.temp_bytes, (const unsigned long long*)w.keys, w.keys_sorted, (const int32_t*)w.iota, w.idx_sorted,
                                  (size_t)n, 0, 63, s, false);
    if (e != hipSuccess) return (int)e;
    int32_t *head_raw = w.iota, *head = (int32_t*)w.keys, *id = (int32_t*)w.keys + n;          // (keys and iota are spent)
    hipLaunchKernelGGL(pcl_voxel_heads_kernel, grid, block, 0, s, (const unsigned long long*)w.keys_sorted, (const int32_t*)w.idx_sorted, m, head_raw,
                       w.flag);
    PCL_LAUNCH_CHECK();
    e = rocprim::inclusive_scan(w.temp, w.temp_bytes, (const int32_t*)head_raw, head, (size_t)n, rocprim::maximum<int32_t>(), s, false);
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(w.temp, w.temp_bytes, (const int32_t*)w.flag, id, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s, false);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_voxel_finish_kernel, grid, block, 0, s, (const unsigned long long*)w.keys_sorted, (const int32_t*)w.idx_sorted,
                       (const int32_t*)head, (const int32_t*)id, (const int32_t*)w.flag, m, cell, count, first, nvoxels);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the centroids
// One thread per point, whole waves (no early return: the lanes exchange values).  A lane past n, or one whose voxel number lies outside
// [0, nvoxels), carries voxel -1 and adds nothing.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_sums_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, int n,
                                                                  const int32_t* __restrict__ cell, int nvoxels, long long* __restrict__ sums,
                                                                  int32_t* __restrict__ bad)
{
    const int i = blockIdx.x * PCL_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int v = -1;
    long long q[6] = {0, 0, 0, 0, 0, 0};
    if (i < n) {
        v = cell[i];
        if (v < 0 || v >= nvoxels) v = -1;
        int flags = 0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const float a = c < 3 ? xyz[3 * (int64_t)i + c] : rgb[3 * (int64_t)i + c - 3];
            const int f = pcl_voxel_value_bad(a);
            flags |= f;
            q[c] = f ? 0ll : llrint((double)a * 65536.0);
        }
        if (flags) atomicOr(bad, flags);
    }
    // runs of neighbouring lanes with one voxel: a lane starts one where its left neighbour's voxel differs
    const int left = __shfl_up(v, 1, 64);
    const unsigned long long starts = __ballot(lane == 0 || left != v);
    if (starts != ~0ull) {                                                        // (every lane its own run: nothing to combine)
        const int run = __popcll(starts & (~0ull >> (63 - lane)));                // runs that start at or before this lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int other = __shfl_up(run, d, 64);
            const bool same = lane >= d && other == run;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const long long add = __shfl_up(q[c], d, 64);
                if (same) q[c] += add;
            }
        }
    }
    const bool last = lane == 63 || ((starts >> (lane + 1)) & 1ull);              // the run ends here: this lane holds its sum
    // To memory with NEIGHBOURING lanes on neighbouring words of a voxel's 48-byte row (through LDS: lane l of pass k takes word
    // 64 k + l of its wave's 64 x 6): contiguous segments are what the atomic units want, one lane per row is the slow shape
    // (cdna_hip_programming.md, Guideline 12), and a cloud in random order is all such rows.
    __shared__ long long lq[PCL_BLOCK * 6];
    __shared__ int lv[PCL_BLOCK];
    const int w0 = threadIdx.x & ~63;
    lv[threadIdx.x] = last ? v : -1;
#pragma unroll
    for (int c = 0; c < 6; c++) lq[6 * threadIdx.x + c] = q[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int e = 64 * k + lane, pt = e / 6, c = e - 6 * pt;
        const int dst = lv[w0 + pt];
        if (dst >= 0) atomicAdd((unsigned long long*)&sums[6 * (int64_t)dst + c], (unsigned long long)lq[6 * w0 + e]);
    }
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_centroid_kernel(const long long* __restrict__ sums, const int32_t* __restrict__ count, int nvoxels,
                                                                      float* __restrict__ xyz_out, float* __restrict__ rgb_out)
{
    const int v = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (v >= nvoxels) return;
    const int cnt = count[v];
    const double den = (double)cnt * 65536.0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const float a = cnt > 0 ? (float)((double)sums[6 * (int64_t)v + c] / den) : 0.f;
        if (c < 3) xyz_out[3 * (int64_t)v + c] = a;
        else rgb_out[3 * (int64_t)v + c - 3] = a;
    }
}

extern "C" int pcl_voxel_centroids(const float* xyz, const float* rgb, int64_t n, const int32_t* cell, const int32_t* count, int64_t nvoxels,
                                   float* xyz_out, float* rgb_out, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!xyz || !rgb || !cell || !count || !xyz_out || !rgb_out || !bad || !workspace || n <= 0 || n > PCL_MAX_POINTS || nvoxels <= 0 || nvoxels > n)
        return PCL_EINVAL;
    VoxelWs w;
    if (workspace_bytes < voxel_layout(workspace, n, &w)) return PCL_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.sums, 0, (size_t)nvoxels * 6 * 8, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_voxel_sums_kernel, dim3((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, s, xyz, rgb, (int)n, cell,
                       (int)nvoxels, w.sums, bad);
    PCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pcl_voxel_centroid_kernel, dim3((unsigned)((nvoxels + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, s,
                       (const long long*)w.sums, count, (int)nvoxels, xyz_out, rgb_out);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- density weights
// (a voxel number outside [0, nvoxels) weighs 0)
__global__ void __launch_bounds__(PCL_BLOCK) pcl_density_weights_kernel(const int32_t* __restrict__ cell, const int32_t* __restrict__ count, int n,
                                                                       int nvoxels, int cap, float* __restrict__ w)
{
    const int i = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = cell[i];
    float out = 0.f;
    if (v >= 0 && v < nvoxels) {
        const int cnt = count[v];
        out = cnt <= cap ? 1.f : (float)((double)cap / (double)cnt);
    }
    w[i] = out;
}

extern "C" int pcl_density_weights(const int32_t* cell, const int32_t* count, int64_t n, int64_t nvoxels, int64_t cap, float* w, void* stream)
{
    if (!cell || !count || !w || n <= 0 || n > PCL_MAX_POINTS || nvoxels <= 0 || nvoxels > n || cap < 1) return PCL_EINVAL;
    const int c = cap > 0x7fffffff ? 0x7fffffff : (int)cap;                     // (counts are int32: a larger cap trims nothing either)
    hipLaunchKernelGGL(pcl_density_weights_kernel, dim3((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream, cell,
                       count, (int)n, (int)nvoxels, c, w);
    PCL_LAUNCH_CHECK();
    return 0;
}
