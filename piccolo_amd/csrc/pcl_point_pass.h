// pcl_point_pass.h — the per-point pass that pcl_residual.hip and pcl_info.hip are built from: one pose per block in SGPRs, the cloud walked
// in 512-slot steps two ADJACENT packed slots per lane, and for every pair the weighted instance of pcl_sample2 with UNIT weight on fresh
// accumulators — so a lane holds exactly the numbers the loss kernel would have added for its two points, and a kernel says only what
// becomes of them.  Host side: the argument checks and the deal of steps to chunks that the entry points over such a kernel share.
// Outside the loss-kernel hash: the four files it covers are included, never edited.
#pragma once
#include "pcl_host.h"
#include "pcl_sample_device.h"

#define PCL_PASS_STEP (2 * PCL_BLOCK)      // packed slots per block iteration: two per lane
#define PCL_PASS_MAX_CHUNKS 1024

struct PclPassArgs {
    const float* cloud;      // 6 planes of `stride` floats: x, y, z, -r, -g, -b (colour sets: 3 + 3 * sets planes)
    int64_t n, stride;
    const void* pano;
    PclDims dims;
    const float* trans;      // pose b: trans + b * pose_stride, rot + b * pose_stride (yaw, pitch, roll)
    const float* rot;
    int pose_stride, B;
    int steps_base, steps_rem;   // the cloud's ceil(n / PCL_PASS_STEP) steps dealt out evenly: chunk c has steps_base + (c < steps_rem)
};

// Row i = pose i against panorama i: the panorama addresses of the kernels that take one image per pose travel as kernel arguments, up to
// PCL_RES_MAX_IMAGES per launch (pcl_residual.hip's residual rows, pcl_info.hip's and pcl_gn.hip's images instances)
#define PCL_RES_MAX_IMAGES 64
struct PclResPanos { unsigned long long p[PCL_RES_MAX_IMAGES]; };

// The pose as six SGPR pairs (R0,R1)(R2,R3)(R4,R5)(R6,R7)(R8,t0)(t1,t2): every lane computes the same R from yaw / pitch / roll
// (pcl_rot_from_ypr, what pcl_sampling_loss's pose records hold), the first one's is read.  pose_ok (wave-uniform): R and t finite.
__device__ __forceinline__ PclPose6 pcl_pass_pose(const PclPassArgs& a, unsigned b, bool& pose_ok)
{
    const float* __restrict__ tp = a.trans + (int64_t)b * a.pose_stride;
    const float* __restrict__ rp = a.rot + (int64_t)b * a.pose_stride;
    float v[12];
    pcl_rot_from_ypr(rp[0], rp[1], rp[2], v);
    v[9] = tp[0]; v[10] = tp[1]; v[11] = tp[2];
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v[k])));
    pose_ok = true;
#pragma unroll
    for (int k = 0; k < 12; k++) pose_ok = pose_ok && fabsf(v[k]) <= 3.402823466e38f;
    return PclPose6{(f2){v[0], v[1]}, (f2){v[2], v[3]}, (f2){v[4], v[5]}, (f2){v[6], v[7]}, (f2){v[8], v[9]}, (f2){v[10], v[11]}};
}

// The cloud a block walks and how its steps are dealt to chunks: what PclPassArgs holds for the one cloud of a call, and what a block of a
// rooms launch takes from its room's record instead (wave-uniform: the record is selected by the block index alone)
struct PclPassCloud {
    const float* cloud;
    int64_t n, stride;
    int steps_base, steps_rem;
};

// Block (chunk, pose b) walks its chunk's steps of cloud `c` at pose b against `pano_b` and, with CS, colour set `set` of a cloud of `sets`
// colour sets (a uniform plane offset on the one cloud resource, as in the loss kernel).  For every pair of slots i0, i0 + 1:
//   per_pair(i0, j, valid0, valid1, acc, pose_ok)      j: the slot the pair was loaded from (a pair never leaves its padded plane)
// with acc the forward (GRAD: and gradient) sums of pcl_sample2 for that pair alone: 0 l, 1 mask bit, GRAD: 2-4 g, 5-7 tau.
// pcl_point_pass below is block blockIdx.x = chunk * a.B + b over the call's one cloud, a's own.
// DEPTH (the depth mask): the block also takes the call's z-buffers `dz` ([a.B][Hd * Wd] words behind one buffer
// resource, pose b's at a wave-uniform scalar offset) and their grid; pcl_project2<FMT, true> issues the two cells' look-ups with the
// texels, the pair is sampled with its valid bits cleared where d2 = pz^2 + rho2 > Z[cell] — the loss kernel's own test (pcl_loss.hip,
// VIS == 2) — so a hidden point's acc is that of a masked one, and per_pair takes the two visibility bits behind its other arguments:
//   per_pair(i0, j, valid0, valid1, acc, pose_ok, vis0, vis1)      valid0 / valid1 still say "a point of the cloud"
// Without the flag nothing of this is compiled and an instance keeps the instruction stream it had.
struct PclPassDepth {
    const uint32_t* zbuf;    // [B][Hd * Wd], built by pcl_launch_zbuffers at the poses the pass evaluates
    PclDepthGrid grid;
};

template <int FMT, bool GRAD, bool CS, bool DEPTH = false, class F>
__device__ __forceinline__ void pcl_point_pass_at(const PclPassArgs& a, const PclPassCloud& c, unsigned b, unsigned chunk, const void* pano_b, int sets,
                                                  unsigned set, F&& per_pair, const PclPassDepth* dz = nullptr)
{
    bool pose_ok;
    const PclPose6 P = pcl_pass_pose(a, b, pose_ok);

    __amdgpu_buffer_rsrc_t tex = pcl_tex_rsrc(pano_b, a.dims.H, a.dims.W, pcl_texel_bytes(FMT));
    __amdgpu_buffer_rsrc_t cld = __builtin_amdgcn_make_buffer_rsrc((void*)c.cloud, 0, CS ? (int)(c.stride * (3 + 3 * sets) * 4) : (int)(c.stride * 6 * 4),
                                                                   0x00020000);
    const int plane = (int)c.stride * 4;
    const int cplane = CS ? (int)(3u + 3u * set) * plane : 3 * plane;      // byte offset of the first colour plane this pose reads (uniform)

    const int first = (int)chunk * c.steps_base + min((int)chunk, c.steps_rem);
    const int nsteps = c.steps_base + ((int)chunk < c.steps_rem ? 1 : 0);
    const int n = (int)c.n, last_pair = (int)c.stride - 2;
    __amdgpu_buffer_rsrc_t zb = __amdgpu_buffer_rsrc_t();
    int zoff = 0;
    if constexpr (DEPTH) {
        // (32 unsigned bits: the B z-buffers together stay below 4 GiB, pcl_depth_check)
        zb = __builtin_amdgcn_make_buffer_rsrc((void*)dz->zbuf, 0, (int)((unsigned)a.B * (unsigned)(dz->grid.last + 1) * 4u), 0x00020000);
        zoff = (int)(b * (unsigned)(dz->grid.last + 1) * 4u);
    }
    for (int s = first; s < first + nsteps; s++) {
        const int i0 = s * PCL_PASS_STEP + 2 * (int)threadIdx.x, i1 = i0 + 1;
        const bool valid0 = i0 < n, valid1 = i1 < n;
        const int j = min(i0, last_pair);                     // (the planes are padded to a multiple of 256 slots: a pair never leaves its plane)
        f2 p[6];
#pragma unroll
        for (int k = 0; k < 6; k++)
            p[k] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(cld, j * 4, (CS && k >= 3) ? cplane + (k - 3) * plane : k * plane, 0));
        PclProj<FMT> pj;
        if constexpr (DEPTH) pcl_project2<FMT, true>(p[0], p[1], p[2], P, tex, a.dims, pj, zb, zoff, &dz->grid);
        else pcl_project2<FMT>(p[0], p[1], p[2], P, tex, a.dims, pj);
        f2 acc[PCL_NACC];
#pragma unroll
        for (int k = 0; k < PCL_NACC; k++) acc[k] = F2(0.f);
        int count = 0;
        if constexpr (DEPTH) {
            // visible iff d^2 <= (zmin (1 + tau))^2 = the cell; an empty cell holds +inf (no short-circuit, as in the loss kernel)
            const f2 d2 = pcl_fma2(pj.pz, pj.pz, pj.rho2);
            const bool vis0 = d2.x <= __uint_as_float(pj.zq0), vis1 = d2.y <= __uint_as_float(pj.zq1);
            pcl_sample2<GRAD, FMT, true>(pj, p[3], p[4], p[5], valid0 & vis0, valid1 & vis1, 0ull, 0ull, tex, a.dims, acc, count, F2(1.f));
            per_pair(i0, j, valid0, valid1, acc, pose_ok, vis0, vis1);
        } else {
            pcl_sample2<GRAD, FMT, true>(pj, p[3], p[4], p[5], valid0, valid1, 0ull, 0ull, tex, a.dims, acc, count, F2(1.f));
            per_pair(i0, j, valid0, valid1, acc, pose_ok);
        }
    }
}

template <int FMT, bool GRAD, bool CS, bool DEPTH = false, class F>
__device__ __forceinline__ void pcl_point_pass(const PclPassArgs& a, const void* pano_b, int sets, unsigned set, F&& per_pair,
                                               const PclPassDepth* dz = nullptr)
{
    pcl_point_pass_at<FMT, GRAD, CS, DEPTH>(a, PclPassCloud{a.cloud, a.n, a.stride, a.steps_base, a.steps_rem}, blockIdx.x % (unsigned)a.B,
                                            blockIdx.x / (unsigned)a.B, pano_b, sets, set, per_pair, dz);
}

// What a residual row holds for a point from the pass's forward sums acc[0] = sum, acc[1] = kept (pcl_residual.hip, pcl_depth_info.hip)
__device__ __forceinline__ float pcl_res_value(float sum, float kept, bool pose_ok)
{
    // kept: ||d||.  Not kept: -1.  A pose that holds a NaN or an infinity projects every point to NaN; the clip of the angles (v_med3) then
    // turns the NaN into a number and the point samples a corner of the panorama as if it had been seen there: such a point is neither
    // kept nor masked here, it is NaN — nobody takes a pose that sees nothing for one whose points agree or are masked
    if (!pose_ok || sum != sum) return __builtin_nanf("");
    return kept != 0.f ? sum : -1.f;
}

// ---- host side

// The chunks of an n-point cloud whose chunks walk at least `min_steps` steps where the cloud has them (0: n out of range), and its steps
static inline int64_t pcl_pass_chunks(int64_t n, int min_steps, int64_t* steps_out)
{
    if (n <= 0 || n > PCL_MAX_POINTS) return 0;
    const int64_t steps = (n + PCL_PASS_STEP - 1) / PCL_PASS_STEP;
    int64_t nchunks = (steps + min_steps - 1) / min_steps;
    if (nchunks > PCL_PASS_MAX_CHUNKS) nchunks = PCL_PASS_MAX_CHUNKS;
    if (steps_out) *steps_out = steps;
    return nchunks;
}

// What every entry point over the pass checks and fills; the grid is *nchunks_out x B blocks
static inline int pcl_pass_args(PclPassArgs* a, const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const float* trans,
                                const float* rot, int pose_stride, int B, int min_steps, int64_t* nchunks_out)
{
    if (!cloud || !pano || !trans || !rot) return PCL_EINVAL;
    if (n <= 0 || n > PCL_MAX_POINTS || B <= 0 || H <= 0 || W <= 0 || pose_stride < 3) return PCL_EINVAL;
    if (pano_format != PCL_PANO_F32 && pano_format != PCL_PANO_U8 && pano_format != PCL_PANO_F16) return PCL_EINVAL;      // (U8P / U8V: trim only)
    if ((int64_t)(H + 2) * (W + 2) * pcl_texel_bytes(pano_format) >= ((int64_t)1 << 31)) return PCL_EINVAL;
    int64_t steps;
    const int64_t nchunks = pcl_pass_chunks(n, min_steps, &steps);
    if (nchunks * B > 0x7fffffffll) return PCL_EINVAL;
    a->cloud = cloud; a->n = n; a->stride = pcl_cloud_stride(n);
    a->pano = pano; a->dims = pcl_make_dims(H, W, pano_format);
    a->trans = trans; a->rot = rot; a->pose_stride = pose_stride; a->B = B;
    a->steps_base = (int)(steps / nchunks); a->steps_rem = (int)(steps % nchunks);
    *nchunks_out = nchunks;
    return 0;
}

// f(std::integral_constant<int, FMT>{}) for the three texel formats the pass samples
template <class F>
static inline void pcl_with_pass_fmt(int pano_format, F&& f)
{
    if (pano_format == PCL_PANO_U8) return f(std::integral_constant<int, PCL_PANO_U8>{});
    if (pano_format == PCL_PANO_F16) return f(std::integral_constant<int, PCL_PANO_F16>{});
    f(std::integral_constant<int, PCL_PANO_F32>{});
}
