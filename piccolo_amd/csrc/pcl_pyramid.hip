// pcl_pyramid.hip — the panorama pyramid of the coarse-to-fine refinement chain (build-defined; the rule: include/piccolo_hip.h) and the
// plateau reset a chain may call when it moves to the next level.
//   pyramid : (H,W,3) float image of exact levels k/255 -> levels 1..L, each the zero-bordered texels the loss kernel streams (F16 / U8 /
//             F32, byte for byte what pcl_pano_pack_* writes for the level's float image) and, optionally, the float level images
// ONE launch for all levels: a block owns a 32 x 32 tile of source pixels (32 is a multiple of 2^levels, and H and W are multiples of
// 2^levels: every 2 x 2 block of every level lies in one tile, wholly inside the image or wholly outside), a thread makes the level-1
// pixel of its own 2 x 2 source block in registers, and the tile goes down through the levels in LDS as packed 32-bit RGB levels
// (r | g << 8 | b << 16: the RGBA8 texel).
#include "pcl_gd_state.h"
#include "pcl_host.h"

#define PCL_PYR_MAX_LEVELS 4
#define PCL_PYR_TILE 32                                 // source pixels per tile side; PCL_BLOCK threads x one 2 x 2 block each
static_assert(PCL_PYR_TILE * PCL_PYR_TILE == 4 * PCL_BLOCK, "one 2 x 2 source block per thread");
static_assert(PCL_PYR_TILE % (1 << PCL_PYR_MAX_LEVELS) == 0, "a tile holds whole blocks of the coarsest level");

static bool pyr_format_ok(int f) { return f == PCL_PANO_F16 || f == PCL_PANO_U8 || f == PCL_PANO_F32; }
static bool pyr_shape_ok(int H, int W, int levels)
{
    return H > 0 && W > 0 && levels >= 1 && levels <= PCL_PYR_MAX_LEVELS && H % (1 << levels) == 0 && W % (1 << levels) == 0;
}

// where the levels lie: level l's texels at byte tex[l - 1] of `texels` (256-byte aligned, the region rounded up to 256 bytes), its float
// image at float img[l - 1] of `images`
struct PclPyrArgs {
    int levels;
    int fmt[PCL_PYR_MAX_LEVELS];
    long long tex[PCL_PYR_MAX_LEVELS];
    long long img[PCL_PYR_MAX_LEVELS];
};

static size_t pyr_layout(int H, int W, int levels, const int* formats, PclPyrArgs* a)
{
    size_t off = 0, img = 0;
    a->levels = levels;
    for (int l = 1; l <= PCL_PYR_MAX_LEVELS; l++) {
        a->fmt[l - 1] = l <= levels ? formats[l - 1] : PCL_PANO_U8;
        a->tex[l - 1] = (long long)off; a->img[l - 1] = (long long)img;
        if (l > levels) continue;
        off += pcl_align256(pcl_pano_bytes(H >> l, W >> l, formats[l - 1]));
        img += (size_t)(H >> l) * (size_t)(W >> l) * 3;
    }
    return off;
}

extern "C" size_t pcl_pano_pyramid_bytes(int H, int W, int levels, const int* formats)
{
    if (!formats || !pyr_shape_ok(H, W, levels)) return 0;
    for (int l = 0; l < levels; l++)
        if (!pyr_format_ok(formats[l])) return 0;
    PclPyrArgs a;
    return pyr_layout(H, W, levels, formats, &a);
}

// The rule, on four packed pixels of the finer level.  Black (word 0) is "no data": the mean is over the non-black pixels, rounded to
// nearest with ties up; a block with data never comes out black (the only reachable case: three pixels with channel sums 1, 1, 1, where
// every channel that holds the largest sum gets level 1).
__device__ __forceinline__ uint32_t pcl_pyr_reduce(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t cnt = (a != 0u) + (b != 0u) + (c != 0u) + (d != 0u);
    if (cnt == 0u) return 0u;
    uint32_t s[3], k[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int sh = 8 * ch;
        s[ch] = ((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u);
        const uint32_t t = s[ch] + (cnt >> 1);
        k[ch] = cnt == 1u ? t : cnt == 2u ? t >> 1 : cnt == 4u ? t >> 2 : t / 3u;
    }
    if ((k[0] | k[1] | k[2]) == 0u) {
        const uint32_t mx = max(s[0], max(s[1], s[2]));
#pragma unroll
        for (int ch = 0; ch < 3; ch++) k[ch] = s[ch] == mx ? 1u : 0u;
    }
    return k[0] | k[1] << 8 | k[2] << 16;
}

// one texel of a level in its format (bordered coordinates yp, xp of an (h + 2, w + 2) image), as the pack kernel of that format writes it
__device__ __forceinline__ void pcl_pyr_texel(void* base, int fmt, int64_t i, uint32_t word)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const float r = (float)(word & 255u), g = (float)((word >> 8) & 255u), b = (float)((word >> 16) & 255u);
    if (fmt == PCL_PANO_U8) {
        ((uint32_t*)base)[i] = word;
    } else if (fmt == PCL_PANO_F16) {
        h2 rg = {(_Float16)r, (_Float16)g}, b0 = {(_Float16)b, (_Float16)0.f};
        ((pcl_i2*)base)[i] = (pcl_i2){__builtin_bit_cast(int, rg), __builtin_bit_cast(int, b0)};
    } else {
        ((pcl_f4*)base)[i] = (pcl_f4){__fdiv_rn(r, 255.f), __fdiv_rn(g, 255.f), __fdiv_rn(b, 255.f), 0.f};
    }
}

// Level l's outputs of one block: the pixel (y, x) this thread made (`mine`), and — blocks on the image's edge — the zero border next to the
// block's pixels, so that the blocks' rectangles partition the bordered image: every texel is written once.
__device__ __forceinline__ void pcl_pyr_emit(const PclPyrArgs& a, int l, int h, int w, char* __restrict__ texels, float* __restrict__ images, bool mine,
                                             int y, int x, uint32_t word, int ty0, int tx0, int side)
{
    const int fmt = a.fmt[l - 1], Wp = w + 2;
    char* base = texels + a.tex[l - 1];
    if (mine) {
        pcl_pyr_texel(base, fmt, (int64_t)(y + 1) * Wp + (x + 1), word);
        if (images) {
            float* o = images + a.img[l - 1] + ((int64_t)y * w + x) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) o[ch] = __fdiv_rn((float)((word >> (8 * ch)) & 255u), 255.f);
        }
    }
    // this block's pixels are rows [ty0, ty1) x columns [tx0, tx1) of the level; its rectangle of the bordered image takes the border along
    const int ty1 = min(ty0 + side, h), tx1 = min(tx0 + side, w);
    if (ty0 == 0 || tx0 == 0 || ty1 == h || tx1 == w) {
        const int Y0 = ty0 == 0 ? 0 : ty0 + 1, Y1 = ty1 == h ? h + 2 : ty1 + 1, X0 = tx0 == 0 ? 0 : tx0 + 1, X1 = tx1 == w ? w + 2 : tx1 + 1;
        const int cols = X1 - X0, total = (Y1 - Y0) * cols;
        for (int i = threadIdx.x; i < total; i += PCL_BLOCK) {
            const int yp = Y0 + i / cols, xp = X0 + i % cols;
            if (yp == 0 || yp == h + 1 || xp == 0 || xp == w + 1) pcl_pyr_texel(base, fmt, (int64_t)yp * Wp + xp, 0u);
        }
    }
    // the bytes between the end of the level's texels and the next 256-byte boundary: block (0, 0)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const int64_t bytes = (int64_t)(h + 2) * Wp * pcl_texel_bytes(fmt);
        const int pad = (int)((256 - (bytes & 255)) & 255) >> 2;                    // (every texel size is a multiple of 4 bytes)
        if ((int)threadIdx.x < pad) ((uint32_t*)(base + bytes))[threadIdx.x] = 0u;
    }
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pyramid_kernel(const float* __restrict__ img, int H, int W, PclPyrArgs a, char* __restrict__ texels,
                                                                     float* __restrict__ images, int* __restrict__ not_exact)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    // level l's pixels of the tile, in quads: pixel (py, px) of an n x n level tile at ((py >> 1) * (n / 2) + (px >> 1)) * 4 + (py & 1) * 2 + (px & 1),
    // so that the thread of the next level reads its 2 x 2 block as ONE 16-byte access and a wave's reads are contiguous; the 32 lanes of
    // a half-wave of writers (two tile rows) hit 32 different dwords
    __shared__ __attribute__((aligned(16))) uint32_t lds1[PCL_BLOCK], lds2[PCL_BLOCK / 4], lds3[PCL_BLOCK / 16];
    const int t = threadIdx.x;
    const int n1 = PCL_PYR_TILE / 2, py = t / n1, px = t % n1;
    const int y1 = blockIdx.y * n1 + py, x1 = blockIdx.x * n1 + px;                // this thread's level-1 pixel
    const bool in1 = y1 < (H >> 1) && x1 < (W >> 1);
    uint32_t word = 0u;
    if (in1) {
        uint32_t p[4];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            // two neighbouring pixels: 24 contiguous bytes, 8-byte aligned (an even pixel index: W and the column are even)
            const f2* s = (const f2*)(img + ((int64_t)(2 * y1 + r) * W + 2 * x1) * 3);
            const f2 v0 = s[0], v1 = s[1], v2 = s[2];
            const float f[6] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y};
            p[2 * r] = 0u; p[2 * r + 1] = 0u;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const float k = rintf(f[c] * 255.f);
                // exact iff dividing the level back gives the value (pcl_pano_pack_u8's test)
                bad = bad || !(k >= 0.f && k <= 255.f) || __fdiv_rn(k, 255.f) != f[c];
                p[2 * r + c / 3] |= ((uint32_t)k & 255u) << (8 * (c % 3));
            }
        }
        if (bad) *not_exact = 1;
        word = pcl_pyr_reduce(p[0], p[1], p[2], p[3]);
    }
    lds1[((py >> 1) * (n1 / 2) + (px >> 1)) * 4 + (py & 1) * 2 + (px & 1)] = word;
    pcl_pyr_emit(a, 1, H >> 1, W >> 1, texels, images, in1, y1, x1, word, blockIdx.y * n1, blockIdx.x * n1, n1);
    if (a.levels < 2) return;                                                      // (uniform)
    __syncthreads();

    const int n2 = n1 / 2, qy = t / n2, qx = t % n2;
    const int y2 = blockIdx.y * n2 + qy, x2 = blockIdx.x * n2 + qx;
    const bool in2 = t < n2 * n2 && y2 < (H >> 2) && x2 < (W >> 2);
    word = 0u;
    if (t < n2 * n2) {
        const pcl_i4 q = ((const pcl_i4*)lds1)[t];
        word = pcl_pyr_reduce((uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w);
        lds2[((qy >> 1) * (n2 / 2) + (qx >> 1)) * 4 + (qy & 1) * 2 + (qx & 1)] = word;
    }
    pcl_pyr_emit(a, 2, H >> 2, W >> 2, texels, images, in2, y2, x2, word, blockIdx.y * n2, blockIdx.x * n2, n2);
    if (a.levels < 3) return;
    __syncthreads();

    const int n3 = n2 / 2, ry = t / n3, rx = t % n3;
    const int y3 = blockIdx.y * n3 + ry, x3 = blockIdx.x * n3 + rx;
    const bool in3 = t < n3 * n3 && y3 < (H >> 3) && x3 < (W >> 3);
    word = 0u;
    if (t < n3 * n3) {
        const pcl_i4 q = ((const pcl_i4*)lds2)[t];
        word = pcl_pyr_reduce((uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w);
        lds3[((ry >> 1) * (n3 / 2) + (rx >> 1)) * 4 + (ry & 1) * 2 + (rx & 1)] = word;
    }
    pcl_pyr_emit(a, 3, H >> 3, W >> 3, texels, images, in3, y3, x3, word, blockIdx.y * n3, blockIdx.x * n3, n3);
    if (a.levels < 4) return;
    __syncthreads();

    const int n4 = n3 / 2, sy = t / n4, sx = t % n4;
    const int y4 = blockIdx.y * n4 + sy, x4 = blockIdx.x * n4 + sx;
    const bool in4 = t < n4 * n4 && y4 < (H >> 4) && x4 < (W >> 4);
    word = 0u;
    if (t < n4 * n4) {
        const pcl_i4 q = ((const pcl_i4*)lds3)[t];
        word = pcl_pyr_reduce((uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w);
    }
    pcl_pyr_emit(a, 4, H >> 4, W >> 4, texels, images, in4, y4, x4, word, blockIdx.y * n4, blockIdx.x * n4, n4);
}

extern "C" int pcl_pano_pyramid(const float* img_hwc, int H, int W, int levels, const int* formats, void* texels, float* images, int* not_exact,
                                void* stream)
{
    if (!img_hwc || !formats || !texels || !not_exact || ((uintptr_t)img_hwc & 7)) return PCL_EINVAL;       // (the kernel reads 8-byte pairs)
    if (pcl_pano_pyramid_bytes(H, W, levels, formats) == 0) return PCL_EINVAL;
    PclPyrArgs a;
    pyr_layout(H, W, levels, formats, &a);
    const dim3 grid((unsigned)((W + PCL_PYR_TILE - 1) / PCL_PYR_TILE), (unsigned)((H + PCL_PYR_TILE - 1) / PCL_PYR_TILE));
    hipLaunchKernelGGL(pcl_pano_pyramid_kernel, grid, dim3(PCL_BLOCK), 0, (hipStream_t)stream, img_hwc, H, W, a, (char*)texels, images, not_exact);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---- the plateau scheduler starts over (a chain that moves to another panorama level compares losses of another image): `best` and
// `num_bad` of every candidate, in both copies of the state, as pcl_gd_init writes them; lr, Adam's moments, the step count and the pose
// records stay
__global__ void pcl_gd_plateau_reset_kernel(PclGdPose* st0, PclGdPose* st1, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    st0[b].best = __builtin_inf(); st0[b].num_bad = 0;
    st1[b].best = __builtin_inf(); st1[b].num_bad = 0;
}

extern "C" int pcl_gd_plateau_reset(void* state, int B, void* stream)
{
    if (!state || B <= 0) return PCL_EINVAL;
    hipLaunchKernelGGL(pcl_gd_plateau_reset_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, gd_poses(state, B, 0), gd_poses(state, B, 1), B);
    PCL_LAUNCH_CHECK();
    return 0;
}
