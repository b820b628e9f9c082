// pcl_align.hip — from a voxel grid to the cloud's up direction (additive to ABI 12; build-defined, include/piccolo_hip.h; DESIGN.md
// section 2d): exact second moments per voxel, plane normals, an integer vote for the up axis and the wall direction, and the rigid
// transform that applies the answer.
//
//   pcl_voxel_moments          q(a) = llrint((double)a 65536), d_i = q(x_i) - q(x_first[v]); per voxel S1 = sum d (3) and S2 = sum d_a d_b
//                              (xx xy xz yy yz zz) as exact int64: the bits depend on no launch shape.  (The point order chooses a
//                              voxel's first point, hence the moments; the scatter matrix they give is the same, exactly.)  Range: the points of
//                              one cell lie less than a voxel apart, so |d| <= voxel 65536 + 1 (the + 1: two roundings); at voxel <= 2
//                              that is 131073, d^2 < 2^34.0001, and PCL_MAX_POINTS = 2^27 of them stay below 2^61.0001 < 2^63.  A voxel above
//                              2 m is refused.  Runs of neighbouring lanes with one voxel are combined in the wave and a voxel's 72-byte
//                              row is written contiguously through LDS, as pcl_voxel_sums_kernel does (cdna_hip_programming.md,
//                              Guideline 12); every atomic is a vector 64-bit integer add.
//   pcl_voxel_normals          A = count S2 - S1 S1^T exactly, in 128-bit integers; every entry rounded ONCE to double and divided by
//                              ((double)count (double)count 2^32): the covariance in m^2.  Cyclic Jacobi in double, PCL_ALIGN_SWEEPS sweeps
//                              whatever the data (a zero off-diagonal entry only skips its rotation).
//   pcl_align_vote             integer histograms and integer sums of the normals: one set of bits whatever the launch shape.
//   pcl_align_transform_cloud  out = R (x - a) in fp32: d = x - a, out_r = (R_r0 d_0 + R_r1 d_1) + R_r2 d_2.
// Contraction is off in the whole file: the vote is restated operation by operation by tests/align_helpers.py.
#include "pcl_host.h"

#pragma clang fp contract(off)

#define PCL_ALIGN_SWEEPS 8
#define PCL_ALIGN_GRID 64                        // the up vote's histogram: GRID x GRID bins over the gnomonic plane
#define PCL_ALIGN_ROUNDS 3                       // rounds of the cone mean
#define PCL_ALIGN_YAW_BINS 360                   // 0.25 degrees each over [0, 90)
#define PCL_ALIGN_COS_CONE 0.99619469809174555   // cos 5 degrees
#define PCL_ALIGN_SIN_WALL 0.17364817766693033   // sin 10 degrees: a wall's normal lies within 10 degrees of the horizontal plane
#define PCL_ALIGN_YAW_HALF 3.0                   // degrees each side of the heaviest bin's centre
#define PCL_ALIGN_Q 1048576.0                    // 2^20: a normal's component as an integer
#define PCL_ALIGN_DEG 57.295779513082323         // 180 / pi

// (pcl_voxel.hip's rule for a coordinate: 1 NaN or infinite, 4 magnitude >= 32768)
__device__ __forceinline__ int pcl_align_value_bad(float a)
{
    if (!(fabsf(a) <= 3.402823466e38f)) return 1;
    return fabsf(a) >= 32768.f ? 4 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- the moments
// One thread per point, whole waves (no early return: the lanes exchange values).  A lane past n, one whose voxel number lies outside
// [0, nvoxels), one with a bad coordinate, and one whose voxel's first point lies outside [0, n) or is bad, carries voxel -1 and adds nothing.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_moments_kernel(const float* __restrict__ xyz, int n, const int32_t* __restrict__ cell,
                                                                     const int64_t* __restrict__ first, int nvoxels,
                                                                     unsigned long long* __restrict__ moments, int32_t* __restrict__ bad)
{
    const int i = blockIdx.x * PCL_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int v = -1;
    unsigned long long q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        v = cell[i];
        if (v < 0 || v >= nvoxels) v = -1;
        int flags = 0;
        long long d[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float a = xyz[3 * (int64_t)i + c];
            const int f = pcl_align_value_bad(a);
            flags |= f;
            d[c] = f ? 0ll : llrint((double)a * 65536.0);
        }
        if (flags) {
            atomicOr(bad, flags);
            v = -1;
        }
        if (v >= 0) {
            const int64_t p = first[v];
            if (p < 0 || p >= (int64_t)n) v = -1;
            else {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float a = xyz[3 * p + c];
                    if (pcl_align_value_bad(a)) v = -1;                           // (that point's own lane reports it)
                    else d[c] -= llrint((double)a * 65536.0);
                }
            }
        }
        if (v >= 0) {                                                             // (unsigned: a caller's wrong grid wraps, it does not trap)
            const unsigned long long x = (unsigned long long)d[0], y = (unsigned long long)d[1], z = (unsigned long long)d[2];
            q[0] = x, q[1] = y, q[2] = z;
            q[3] = x * x, q[4] = x * y, q[5] = x * z, q[6] = y * y, q[7] = y * z, q[8] = z * z;
        }
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
            for (int c = 0; c < 9; c++) {
                const unsigned long long add = __shfl_up(q[c], d, 64);
                if (same) q[c] += add;
            }
        }
    }
    const bool last = lane == 63 || ((starts >> (lane + 1)) & 1ull);              // the run ends here: this lane holds its sum
    // to memory with neighbouring lanes on neighbouring words of a voxel's 72-byte row: lane l of pass k takes word 64 k + l of its
    // wave's 64 x 9
    __shared__ unsigned long long lq[PCL_BLOCK * 9];
    __shared__ int lv[PCL_BLOCK];
    const int w0 = threadIdx.x & ~63;
    lv[threadIdx.x] = last ? v : -1;
#pragma unroll
    for (int c = 0; c < 9; c++) lq[9 * threadIdx.x + c] = q[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int e = 64 * k + lane, pt = e / 9, c = e - 9 * pt;
        const int dst = lv[w0 + pt];
        if (dst >= 0) atomicAdd(&moments[9 * (int64_t)dst + c], lq[9 * w0 + e]);
    }
}

extern "C" int pcl_voxel_moments(const float* xyz, int64_t n, double voxel, const int32_t* cell, const int64_t* first, int64_t nvoxels,
                                 int64_t* moments, int32_t* bad, void* stream)
{
    if (!xyz || !cell || !first || !moments || !bad || n <= 0 || n > PCL_MAX_POINTS || nvoxels <= 0 || nvoxels > n) return PCL_EINVAL;
    if (!(voxel > 0.0 && voxel <= 2.0)) return PCL_EINVAL;                       // (the range rule above; NaN fails both)
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(moments, 0, (size_t)nvoxels * 9 * 8, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_voxel_moments_kernel, dim3((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, s, xyz, (int)n, cell, first,
                       (int)nvoxels, (unsigned long long*)moments, bad);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the normals
// a 128-bit integer rounded once (to nearest, ties to even) to double: its top 64 bits with the rest folded into a sticky last bit — 64
// bits are 11 more than a double keeps, so the one rounding of the 64-bit conversion is the rounding of the whole
__device__ __forceinline__ double pcl_align_i128_to_double(__int128 a)
{
    const bool neg = a < 0;
    const unsigned __int128 m = neg ? -(unsigned __int128)a : (unsigned __int128)a;
    const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
    double r;
    if (hi == 0ull) r = (double)lo;
    else {
        const int lz = __clzll((long long)hi);                                    // (hi != 0: 0..63)
        const unsigned long long top = lz ? (hi << lz) | (lo >> (64 - lz)) : hi;
        const unsigned long long rest = lz ? lo << lz : lo;
        r = ldexp((double)(top | (rest != 0ull ? 1ull : 0ull)), 64 - lz);
    }
    return neg ? -r : r;
}

// one Jacobi rotation that zeroes a[p][q] of the symmetric a (r the third index), accumulated into the eigenvector columns of v
#define PCL_ALIGN_ROTATE(p, q, r)                                                 \
    if (a[p][q] != 0.0) {                                                         \
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);               \
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); \
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;                     \
        const double apq = a[p][q], arp = a[r][p], arq = a[r][q];                 \
        a[p][p] -= t * apq;                                                       \
        a[q][q] += t * apq;                                                       \
        a[p][q] = a[q][p] = 0.0;                                                  \
        a[r][p] = a[p][r] = c * arp - sn * arq;                                   \
        a[r][q] = a[q][r] = sn * arp + c * arq;                                   \
        _Pragma("unroll") for (int k = 0; k < 3; k++) {                           \
            const double vp = v[k][p], vq = v[k][q];                              \
            v[k][p] = c * vp - sn * vq;                                           \
            v[k][q] = sn * vp + c * vq;                                           \
        }                                                                         \
    }

__global__ void __launch_bounds__(PCL_BLOCK) pcl_voxel_normals_kernel(const int64_t* __restrict__ moments, const int32_t* __restrict__ count,
                                                                     int nvoxels, int min_count, float* __restrict__ normal,
                                                                     float* __restrict__ planarity, float* __restrict__ eig)
{
    const int vox = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (vox >= nvoxels) return;
    const int cnt = count[vox];
    float nout[3] = {0.f, 0.f, 0.f}, pout = 0.f, eout[3] = {0.f, 0.f, 0.f};
    if (cnt >= min_count) {
        long long m[9];
#pragma unroll
        for (int c = 0; c < 9; c++) m[c] = moments[9 * (int64_t)vox + c];
        const double den = (double)cnt * (double)cnt * 4294967296.0;
        double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        int s2 = 3;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p; q < 3; q++, s2++) {
                const __int128 e = (__int128)cnt * (__int128)m[s2] - (__int128)m[p] * (__int128)m[q];
                a[p][q] = a[q][p] = pcl_align_i128_to_double(e) / den;
            }
        for (int sweep = 0; sweep < PCL_ALIGN_SWEEPS; sweep++) {
            PCL_ALIGN_ROTATE(0, 1, 2)
            PCL_ALIGN_ROTATE(0, 2, 1)
            PCL_ALIGN_ROTATE(1, 2, 0)
        }
        // ascending eigenvalues; on equal values the lower column first
        double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
        int i0 = 0, i1 = 1, i2 = 2;
        if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; const int k = i0; i0 = i1; i1 = k; }
        if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; const int k = i1; i1 = i2; i2 = k; }
        if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; const int k = i0; i0 = i1; i1 = k; }
        (void)i1, (void)i2;
        if (l2 > 0.0) {
            double nx = i0 == 0 ? v[0][0] : i0 == 1 ? v[0][1] : v[0][2];
            double ny = i0 == 0 ? v[1][0] : i0 == 1 ? v[1][1] : v[1][2];
            double nz = i0 == 0 ? v[2][0] : i0 == 1 ? v[2][1] : v[2][2];
            const double len = sqrt(nx * nx + ny * ny + nz * nz);
            nx /= len, ny /= len, nz /= len;
            double big = nx;                                                      // the component of largest magnitude (the first of equals)
            if (fabs(ny) > fabs(big)) big = ny;
            if (fabs(nz) > fabs(big)) big = nz;
            if (big < 0.0) nx = -nx, ny = -ny, nz = -nz;
            nout[0] = (float)nx, nout[1] = (float)ny, nout[2] = (float)nz;
            pout = (float)((l1 - l0) / l2);
            eout[0] = (float)l0, eout[1] = (float)l1, eout[2] = (float)l2;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) normal[3 * (int64_t)vox + c] = nout[c];
    planarity[vox] = pout;
    if (eig) {
#pragma unroll
        for (int c = 0; c < 3; c++) eig[3 * (int64_t)vox + c] = eout[c];
    }
}

extern "C" int pcl_voxel_normals(const int64_t* moments, const int32_t* count, int64_t nvoxels, int64_t min_count, float* normal, float* planarity,
                                 float* eig, void* stream)
{
    if (!moments || !count || !normal || !planarity || nvoxels <= 0 || nvoxels > PCL_MAX_POINTS || min_count < 3) return PCL_EINVAL;
    const int mc = min_count > 0x7fffffff ? 0x7fffffff : (int)min_count;          // (counts are int32)
    hipLaunchKernelGGL(pcl_voxel_normals_kernel, dim3((unsigned)((nvoxels + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream,
                       moments, count, (int)nvoxels, mc, normal, planarity, eig);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the vote
// The workspace, in 8-byte words (zeroed by the call):
#define PCL_ALIGN_W_HIST 0                                              // GRID x GRID bins of the up vote
#define PCL_ALIGN_W_YAW (PCL_ALIGN_GRID * PCL_ALIGN_GRID)               // the wall vote's bins
#define PCL_ALIGN_W_ROUND (PCL_ALIGN_W_YAW + PCL_ALIGN_YAW_BINS)        // per round of the cone mean: sum x, sum y, sum z, weight
#define PCL_ALIGN_W_WALL (PCL_ALIGN_W_ROUND + 4 * PCL_ALIGN_ROUNDS)     // sum cos 4 psi, sum sin 4 psi, their weight, the wall bins' weight
#define PCL_ALIGN_W_KEPT (PCL_ALIGN_W_WALL + 4)                         // the up bins' weight
#define PCL_ALIGN_W_START (PCL_ALIGN_W_KEPT + 1)                        // doubles: the heaviest up bin's direction (3)
#define PCL_ALIGN_W_BEST (PCL_ALIGN_W_START + 3)                        // the heaviest up bin's weight, the heaviest wall bin's, that bin
#define PCL_ALIGN_W_WORDS (PCL_ALIGN_W_BEST + 3)

// the weight of a voxel's vote and its normal folded into the upper half space of +z; false: the voxel does not vote
__device__ __forceinline__ bool pcl_align_voter(const float* __restrict__ normal, const float* __restrict__ planarity, const int32_t* __restrict__ count,
                                                int v, long long& w, double n[3], bool fold)
{
    const int cnt = count[v];
    const float p = planarity[v];
    if (cnt <= 0 || !(p > 0.f && p <= 1.f)) return false;
    w = (long long)cnt * llrint((double)p * 4096.0);
    n[0] = (double)normal[3 * (int64_t)v], n[1] = (double)normal[3 * (int64_t)v + 1], n[2] = (double)normal[3 * (int64_t)v + 2];
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (w <= 0 || !(nn > 0.25 && nn < 4.0)) return false;                         // (a zero or NaN normal)
    if (fold && n[2] < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    return true;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_hist_kernel(const float* __restrict__ normal, const float* __restrict__ planarity,
                                                                  const int32_t* __restrict__ count, int nvoxels, double T,
                                                                  unsigned long long* __restrict__ ws)
{
    const int v = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (v >= nvoxels) return;
    long long w;
    double n[3];
    if (!pcl_align_voter(normal, planarity, count, v, w, n, true) || !(n[2] > 0.0)) return;
    const double gu = n[0] / n[2], gv = n[1] / n[2];
    if (!(gu * gu + gv * gv <= T * T)) return;                                    // within max_tilt of +z
    const double scale = (double)(PCL_ALIGN_GRID / 2) / T;
    int bx = (int)floor((gu + T) * scale), by = (int)floor((gv + T) * scale);
    bx = bx < 0 ? 0 : bx > PCL_ALIGN_GRID - 1 ? PCL_ALIGN_GRID - 1 : bx;
    by = by < 0 ? 0 : by > PCL_ALIGN_GRID - 1 ? PCL_ALIGN_GRID - 1 : by;
    atomicAdd(&ws[PCL_ALIGN_W_HIST + by * PCL_ALIGN_GRID + bx], (unsigned long long)w);
    atomicAdd(&ws[PCL_ALIGN_W_KEPT], (unsigned long long)w);
}

// the heaviest of `bins` int64 bins, the lowest index among equals: one block
__device__ __forceinline__ void pcl_align_heaviest(const unsigned long long* __restrict__ hist, int bins, long long& best_w, int& best_i)
{
    __shared__ long long sw[PCL_BLOCK];
    __shared__ int si[PCL_BLOCK];
    long long bw = -1;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < bins; i += PCL_BLOCK) {                         // (ascending i: a later equal does not replace)
        const long long w = (long long)hist[i];
        if (w > bw) bw = w, bi = i;
    }
    sw[threadIdx.x] = bw, si[threadIdx.x] = bi;
    __syncthreads();
    for (int d = PCL_BLOCK / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const long long ow = sw[threadIdx.x + d];
            const int oi = si[threadIdx.x + d];
            if (ow > sw[threadIdx.x] || (ow == sw[threadIdx.x] && oi < si[threadIdx.x])) sw[threadIdx.x] = ow, si[threadIdx.x] = oi;
        }
        __syncthreads();
    }
    best_w = sw[0], best_i = si[0];
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_start_kernel(double T, unsigned long long* __restrict__ ws)
{
    long long bw;
    int bi;
    pcl_align_heaviest(ws + PCL_ALIGN_W_HIST, PCL_ALIGN_GRID * PCL_ALIGN_GRID, bw, bi);
    if (threadIdx.x != 0) return;
    const double step = T / (double)(PCL_ALIGN_GRID / 2);
    const double gu = ((double)(bi % PCL_ALIGN_GRID) + 0.5) * step - T, gv = ((double)(bi / PCL_ALIGN_GRID) + 0.5) * step - T;
    const double len = sqrt(gu * gu + gv * gv + 1.0);
    double* start = (double*)(ws + PCL_ALIGN_W_START);
    start[0] = gu / len, start[1] = gv / len, start[2] = 1.0 / len;
    ws[PCL_ALIGN_W_BEST] = (unsigned long long)bw;
}

// the estimate a round starts from: the heaviest bin's direction, or the round before's sums, normalised
__device__ __forceinline__ void pcl_align_estimate(const unsigned long long* __restrict__ ws, int round, double e[3])
{
    if (round == 0) {
        const double* start = (const double*)(ws + PCL_ALIGN_W_START);
        e[0] = start[0], e[1] = start[1], e[2] = start[2];
        return;
    }
    const long long* s = (const long long*)(ws + PCL_ALIGN_W_ROUND + 4 * (round - 1));
    const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
    const double len = sqrt(x * x + y * y + z * z);
    e[0] = x / len, e[1] = y / len, e[2] = z / len;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_cone_kernel(const float* __restrict__ normal, const float* __restrict__ planarity,
                                                                  const int32_t* __restrict__ count, int nvoxels, int round,
                                                                  unsigned long long* __restrict__ ws)
{
    const int v = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (v >= nvoxels || (long long)ws[PCL_ALIGN_W_BEST] <= 0) return;             // (no voxel inside the tilt cone: nothing to refine)
    long long w;
    double n[3], e[3];
    if (!pcl_align_voter(normal, planarity, count, v, w, n, true)) return;
    pcl_align_estimate(ws, round, e);
    if (!(n[0] * e[0] + n[1] * e[1] + n[2] * e[2] >= PCL_ALIGN_COS_CONE)) return;
    unsigned long long* s = ws + PCL_ALIGN_W_ROUND + 4 * round;
#pragma unroll
    for (int c = 0; c < 3; c++) atomicAdd(&s[c], (unsigned long long)(w * llrint(n[c] * PCL_ALIGN_Q)));
    atomicAdd(&s[3], (unsigned long long)w);
}

// the minimal rotation taking the unit vector a (a_z > 0) to +z, by Rodrigues with v = a x z and c = a_z: I + [v]x + [v]x^2 / (1 + c)
__device__ __forceinline__ void pcl_align_up_rotation(const double a[3], double r[9])
{
    const double k = 1.0 / (1.0 + a[2]);
    r[0] = 1.0 - (a[0] * a[0]) * k, r[1] = -((a[0] * a[1]) * k), r[2] = -a[0];
    r[3] = r[1], r[4] = 1.0 - (a[1] * a[1]) * k, r[5] = -a[1];
    r[6] = a[0], r[7] = a[1], r[8] = 1.0 - (a[0] * a[0] + a[1] * a[1]) * k;
}

// a voxel's wall vote: its normal after the up rotation, if within 10 degrees of the horizontal plane -> the azimuth folded into [0, 90)
// degrees and (cos, sin) of four times the azimuth (two angle doublings of the unit horizontal direction: no transcendental but the
// one arctangent that names the bin)
__device__ __forceinline__ bool pcl_align_wall(const float* __restrict__ normal, const float* __restrict__ planarity, const int32_t* __restrict__ count,
                                               int v, const unsigned long long* __restrict__ ws, long long& w, double& fold, double& c4, double& s4)
{
    double n[3], e[3], r[9];
    if (!pcl_align_voter(normal, planarity, count, v, w, n, false)) return false;
    pcl_align_estimate(ws, PCL_ALIGN_ROUNDS, e);
    pcl_align_up_rotation(e, r);
    const double x = (r[0] * n[0] + r[1] * n[1]) + r[2] * n[2], y = (r[3] * n[0] + r[4] * n[1]) + r[5] * n[2],
                 z = (r[6] * n[0] + r[7] * n[1]) + r[8] * n[2];
    const double h = sqrt(x * x + y * y);
    if (!(fabs(z) <= PCL_ALIGN_SIN_WALL) || !(h > 0.0)) return false;
    const double c1 = x / h, s1 = y / h;
    const double c2 = c1 * c1 - s1 * s1, s2 = 2.0 * (c1 * s1);
    c4 = c2 * c2 - s2 * s2, s4 = 2.0 * (c2 * s2);
    const double deg = atan2(y, x) * PCL_ALIGN_DEG;
    fold = deg - 90.0 * floor(deg / 90.0);
    return true;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_wall_hist_kernel(const float* __restrict__ normal, const float* __restrict__ planarity,
                                                                       const int32_t* __restrict__ count, int nvoxels,
                                                                       unsigned long long* __restrict__ ws)
{
    const int v = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (v >= nvoxels || (long long)ws[PCL_ALIGN_W_BEST] <= 0) return;
    long long w;
    double fold, c4, s4;
    if (!pcl_align_wall(normal, planarity, count, v, ws, w, fold, c4, s4)) return;
    int b = (int)floor(fold * 4.0);
    b = b < 0 ? 0 : b > PCL_ALIGN_YAW_BINS - 1 ? PCL_ALIGN_YAW_BINS - 1 : b;
    atomicAdd(&ws[PCL_ALIGN_W_YAW + b], (unsigned long long)w);
    atomicAdd(&ws[PCL_ALIGN_W_WALL + 3], (unsigned long long)w);
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_wall_start_kernel(unsigned long long* __restrict__ ws)
{
    long long bw;
    int bi;
    pcl_align_heaviest(ws + PCL_ALIGN_W_YAW, PCL_ALIGN_YAW_BINS, bw, bi);
    if (threadIdx.x != 0) return;
    ws[PCL_ALIGN_W_BEST + 1] = (unsigned long long)bw;
    ws[PCL_ALIGN_W_BEST + 2] = (unsigned long long)bi;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_wall_mean_kernel(const float* __restrict__ normal, const float* __restrict__ planarity,
                                                                       const int32_t* __restrict__ count, int nvoxels,
                                                                       unsigned long long* __restrict__ ws)
{
    const int v = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (v >= nvoxels || (long long)ws[PCL_ALIGN_W_BEST] <= 0 || (long long)ws[PCL_ALIGN_W_BEST + 1] <= 0) return;
    long long w;
    double fold, c4, s4;
    if (!pcl_align_wall(normal, planarity, count, v, ws, w, fold, c4, s4)) return;
    const double centre = ((double)(long long)ws[PCL_ALIGN_W_BEST + 2] + 0.5) * 0.25;
    double diff = fold - centre;
    diff -= 90.0 * rint(diff / 90.0);                                             // (the bins close a circle of 90 degrees)
    if (!(fabs(diff) <= PCL_ALIGN_YAW_HALF)) return;
    atomicAdd(&ws[PCL_ALIGN_W_WALL], (unsigned long long)(w * llrint(c4 * PCL_ALIGN_Q)));
    atomicAdd(&ws[PCL_ALIGN_W_WALL + 1], (unsigned long long)(w * llrint(s4 * PCL_ALIGN_Q)));
    atomicAdd(&ws[PCL_ALIGN_W_WALL + 2], (unsigned long long)w);
}

// (cos, sin) of half the angle whose (cos, sin) = (c, s), the half angle in (-90, 90] degrees
__device__ __forceinline__ void pcl_align_half_angle(double c, double s, double& ch, double& sh)
{
    if (c >= 0.0) {
        ch = sqrt((1.0 + c) / 2.0);
        sh = s / (2.0 * ch);
    } else {
        sh = sqrt((1.0 - c) / 2.0);
        if (s < 0.0) sh = -sh;
        ch = s / (2.0 * sh);
    }
}

__global__ void pcl_align_finish_kernel(const unsigned long long* __restrict__ ws, int yaw, PclAlignOut* __restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PclAlignOut o;
    o.up[0] = 0.0, o.up[1] = 0.0, o.up[2] = 1.0;
#pragma unroll
    for (int c = 0; c < 9; c++) o.rot[c] = c % 4 == 0 ? 1.0 : 0.0;
    o.cos_tilt = 1.0, o.sin_tilt = 0.0, o.cos_yaw = 1.0, o.sin_yaw = 0.0;
    o.weight[0] = (long long)ws[PCL_ALIGN_W_KEPT];
    o.weight[1] = (long long)ws[PCL_ALIGN_W_ROUND + 4 * (PCL_ALIGN_ROUNDS - 1) + 3];
    o.weight[2] = (long long)ws[PCL_ALIGN_W_WALL + 3];
    o.weight[3] = (long long)ws[PCL_ALIGN_W_WALL + 2];
    o.status = 0;
    if ((long long)ws[PCL_ALIGN_W_BEST] <= 0) o.status = 1;
    else {
        double e[3], r[9];
        pcl_align_estimate(ws, PCL_ALIGN_ROUNDS, e);
        pcl_align_up_rotation(e, r);
        o.up[0] = e[0], o.up[1] = e[1], o.up[2] = e[2];
        o.cos_tilt = e[2], o.sin_tilt = sqrt(e[0] * e[0] + e[1] * e[1]);
        if (yaw) {
            const double C = (double)(long long)ws[PCL_ALIGN_W_WALL], S = (double)(long long)ws[PCL_ALIGN_W_WALL + 1];
            const double len = sqrt(C * C + S * S);
            if (o.weight[3] <= 0 || !(len > 0.0)) o.status = 2;
            else {
                double c2, s2;
                pcl_align_half_angle(C / len, S / len, c2, s2);
                pcl_align_half_angle(c2, s2, o.cos_yaw, o.sin_yaw);
                // the rotation by -phi about z, times the up rotation
                double t[9];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    t[c] = o.cos_yaw * r[c] + o.sin_yaw * r[3 + c];
                    t[3 + c] = o.cos_yaw * r[3 + c] - o.sin_yaw * r[c];
                    t[6 + c] = r[6 + c];
                }
#pragma unroll
                for (int c = 0; c < 9; c++) r[c] = t[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 9; c++) o.rot[c] = r[c];
    }
    *out = o;
}

// (one size for every voxel count; 0 for a count no call takes, as every sizing function here answers an empty problem)
extern "C" size_t pcl_align_workspace_bytes(int64_t nvoxels)
{
    return nvoxels <= 0 || nvoxels > PCL_MAX_POINTS ? 0 : pcl_align256((size_t)PCL_ALIGN_W_WORDS * 8);
}

extern "C" int pcl_align_vote(const float* normal, const float* planarity, const int32_t* count, int64_t nvoxels, const PclAlignParams* params,
                              PclAlignOut* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!normal || !planarity || !count || !params || !out || !workspace || nvoxels <= 0 || nvoxels > PCL_MAX_POINTS) return PCL_EINVAL;
    if (!(params->max_tilt > 0.0 && params->max_tilt <= 45.0)) return PCL_EINVAL;
    if (workspace_bytes < pcl_align_workspace_bytes(nvoxels)) return PCL_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const double T = tan(params->max_tilt * 0.017453292519943295);                // (the model's math.tan of the same product)
    unsigned long long* ws = (unsigned long long*)workspace;
    const int m = (int)nvoxels;
    const dim3 grid((unsigned)((nvoxels + PCL_BLOCK - 1) / PCL_BLOCK)), block(PCL_BLOCK);
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)PCL_ALIGN_W_WORDS * 8, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pcl_align_hist_kernel, grid, block, 0, s, normal, planarity, count, m, T, ws);
    PCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pcl_align_start_kernel, dim3(1), block, 0, s, T, ws);
    PCL_LAUNCH_CHECK();
    for (int round = 0; round < PCL_ALIGN_ROUNDS; round++) {
        hipLaunchKernelGGL(pcl_align_cone_kernel, grid, block, 0, s, normal, planarity, count, m, round, ws);
        PCL_LAUNCH_CHECK();
    }
    if (params->yaw) {
        hipLaunchKernelGGL(pcl_align_wall_hist_kernel, grid, block, 0, s, normal, planarity, count, m, ws);
        PCL_LAUNCH_CHECK();
        hipLaunchKernelGGL(pcl_align_wall_start_kernel, dim3(1), block, 0, s, ws);
        PCL_LAUNCH_CHECK();
        hipLaunchKernelGGL(pcl_align_wall_mean_kernel, grid, block, 0, s, normal, planarity, count, m, ws);
        PCL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pcl_align_finish_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)ws, params->yaw ? 1 : 0, out);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the transform
__global__ void __launch_bounds__(PCL_BLOCK) pcl_align_transform_kernel(const float* __restrict__ xyz, int n, const float* __restrict__ rot,
                                                                       const float* __restrict__ trans, float* __restrict__ out)
{
    const int i = blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float d0 = xyz[3 * (int64_t)i] - trans[0], d1 = xyz[3 * (int64_t)i + 1] - trans[1], d2 = xyz[3 * (int64_t)i + 2] - trans[2];
#pragma unroll
    for (int r = 0; r < 3; r++) out[3 * (int64_t)i + r] = (rot[3 * r] * d0 + rot[3 * r + 1] * d1) + rot[3 * r + 2] * d2;
}

extern "C" int pcl_align_transform_cloud(const float* xyz, int64_t n, const float* rot, const float* trans, float* out, void* stream)
{
    if (!xyz || !rot || !trans || !out || n <= 0 || n > PCL_MAX_POINTS) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_align_transform_kernel, dim3((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream, xyz,
                       (int)n, rot, trans, out);
    PCL_LAUNCH_CHECK();
    return 0;
}
