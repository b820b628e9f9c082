// pcl_pack.hip — one-time repacking of the reference's tensors into the layouts the loss kernel streams.
//   cloud : row-major (N,3) xyz + (N,3) rgb  (localize.py:159-164)  -> 6 SoA planes x,y,z,-r,-g,-b, optionally re-ordered
//   pano  : (H,W,3) float image              (localize.py:167-170)  -> zero-bordered (H+2, W+2) RGBA float4
#include "pcl_host.h"

#include <rocprim/device/device_radix_sort.hpp>

extern "C" int pcl_abi_version(void) { return PCL_ABI_VERSION; }

#ifndef PCL_SOURCE_HASH
#define PCL_SOURCE_HASH "unstamped"
#endif
extern "C" const char* pcl_source_hash(void) { return PCL_SOURCE_HASH; }
#ifndef PCL_LIBRARY_HASH
#define PCL_LIBRARY_HASH "unstamped"
#endif
extern "C" const char* pcl_library_hash(void) { return PCL_LIBRARY_HASH; }

extern "C" const char* pcl_error_string(int code)
{
    if (code == 0) return "success";
    if (code == PCL_EINVAL) return "piccolo_hip: invalid argument";
    if (code == PCL_EWORKSPACE) return "piccolo_hip: workspace too small";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "piccolo_hip: unknown error";
}

// plane stride: n rounded up to 256 floats (1 KiB) so every plane starts on a fresh 1-KiB wave-load boundary
extern "C" int64_t pcl_cloud_stride(int64_t n) { return n <= 0 ? 0 : ((n + 255) / 256) * 256; }
extern "C" size_t pcl_cloud_bytes(int64_t n) { return (size_t)pcl_cloud_stride(n) * 6 * sizeof(float); }
extern "C" size_t pcl_pano_bytes(int H, int W, int pano_format)
{
    if (H <= 0 || W <= 0) return 0;
    if (pano_format == PCL_PANO_U8P) return (size_t)((H + 3) >> 1) * (size_t)(W + 2) * 8;       // element rows of row PAIRS
    if (pano_format == PCL_PANO_U8V) return (size_t)(H + 2) * (size_t)(W + 2) * 8;              // every texel with the one below it
    if (pano_format != PCL_PANO_F32 && pano_format != PCL_PANO_U8 && pano_format != PCL_PANO_F16) return 0;
    return (size_t)(H + 2) * (size_t)(W + 2) * (size_t)pcl_texel_bytes(pano_format);
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_cloud_pack_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                                   const int64_t* __restrict__ order, int64_t n,
                                                                   int64_t stride, float* __restrict__ cloud)
{
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= stride) return;
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < n) {
        int64_t j = order ? order[i] : i;
        v[0] = xyz[3 * j]; v[1] = xyz[3 * j + 1]; v[2] = xyz[3 * j + 2];
        v[3] = -rgb[3 * j]; v[4] = -rgb[3 * j + 1]; v[5] = -rgb[3 * j + 2];   // the loss needs c - rgb: store -rgb
    }
#pragma unroll
    for (int k = 0; k < 6; k++) cloud[k * stride + i] = v[k];
}

extern "C" int pcl_cloud_pack(const float* xyz, const float* rgb, const int64_t* order, int64_t n, float* cloud, void* stream)
{
    if (!xyz || !rgb || !cloud || n <= 0) return PCL_EINVAL;
    int64_t stride = pcl_cloud_stride(n);
    hipLaunchKernelGGL(pcl_cloud_pack_kernel, dim3((unsigned)(stride / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream,
                       xyz, rgb, order, n, stride, cloud);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---- per-image colour sets (ABI 10): planes x, y, z, then nsets x (-r, -g, -b), each pcl_cloud_stride(n) floats.  Set k is the
// scalar plane offset (3 + 3 k) x plane of the one buffer resource the kernels already build; the whole cloud stays below 2^31 bytes
// so that every plane offset is a non-negative int.  One set is the 6-plane cloud of pcl_cloud_pack (and its limits).
extern "C" size_t pcl_cloud_sets_bytes(int64_t n, int nsets)
{
    if (n <= 0 || n > PCL_MAX_POINTS || nsets <= 0) return 0;
    if (nsets == 1) return pcl_cloud_bytes(n);
    const int64_t bytes = (int64_t)pcl_cloud_stride(n) * 4 * (3 + 3 * (int64_t)nsets);
    return bytes < ((int64_t)1 << 31) ? (size_t)bytes : 0;
}

#define PCL_PACK_SETS 16        // colour sets per launch of the set-packing kernel (their addresses travel as kernel arguments)
struct PclRgbList { const float* p[PCL_PACK_SETS]; };

// the xyz planes (k0 == 0 only) and the colour planes of sets [k0, k0 + m): every thread one packed slot
__global__ void __launch_bounds__(PCL_BLOCK) pcl_cloud_pack_sets_kernel(const float* __restrict__ xyz, PclRgbList rgb, int k0, int m,
                                                                        const int64_t* __restrict__ order, int64_t n, int64_t stride,
                                                                        float* __restrict__ cloud)
{
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= stride) return;
    const int64_t j = i < n ? (order ? order[i] : i) : 0;
    if (k0 == 0)
        for (int c = 0; c < 3; c++) cloud[c * stride + i] = i < n ? xyz[3 * j + c] : 0.f;
    for (int k = 0; k < m; k++)
        for (int c = 0; c < 3; c++) cloud[(3 + 3 * (int64_t)(k0 + k) + c) * stride + i] = i < n ? -rgb.p[k][3 * j + c] : 0.f;   // -rgb, as pcl_cloud_pack
}

extern "C" int pcl_cloud_pack_sets(const float* xyz, const float* const* rgb_host, int nsets, const int64_t* order, int64_t n, float* cloud,
                                   void* stream)
{
    if (!xyz || !rgb_host || !cloud || n <= 0 || nsets <= 0) return PCL_EINVAL;
    if (pcl_cloud_sets_bytes(n, nsets) == 0) return PCL_EINVAL;
    for (int k = 0; k < nsets; k++)
        if (!rgb_host[k]) return PCL_EINVAL;
    if (nsets == 1) return pcl_cloud_pack(xyz, rgb_host[0], order, n, cloud, stream);
    const int64_t stride = pcl_cloud_stride(n);
    for (int k0 = 0; k0 < nsets; k0 += PCL_PACK_SETS) {
        const int m = nsets - k0 < PCL_PACK_SETS ? nsets - k0 : PCL_PACK_SETS;
        PclRgbList l;
        for (int k = 0; k < PCL_PACK_SETS; k++) l.p[k] = k < m ? rgb_host[k0 + k] : nullptr;
        hipLaunchKernelGGL(pcl_cloud_pack_sets_kernel, dim3((unsigned)(stride / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream, xyz, l, k0, m,
                           order, n, stride, cloud);
        PCL_LAUNCH_CHECK();
    }
    return 0;
}

// ---- per-point weights (build-defined: the reference has none): one more plane of pcl_cloud_stride(n) floats in the packed point order,
// plane[s] = w[order ? order[s] : s], padding slots 0.  A buffer of its own, not a seventh plane of the cloud: the cloud keeps its layout,
// and re-packing into the same buffer changes the weights a captured graph reads.  *bad (device int, caller zeroes it) is set when a
// weight is negative, NaN or infinite — pcl_pano_pack_u8's not_exact pattern.
extern "C" size_t pcl_cloud_weights_bytes(int64_t n) { return n <= 0 || n > PCL_MAX_POINTS ? 0 : (size_t)pcl_cloud_stride(n) * sizeof(float); }

__global__ void __launch_bounds__(PCL_BLOCK) pcl_cloud_pack_weights_kernel(const float* __restrict__ w, const int64_t* __restrict__ order, int64_t n,
                                                                           int64_t stride, float* __restrict__ plane, int32_t* __restrict__ bad)
{
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= stride) return;
    float v = 0.f;
    if (i < n) {
        v = w[order ? order[i] : i];
        if (!(v >= 0.f && v <= 3.402823466e38f)) *bad = 1;               // negative, NaN or infinite
    }
    plane[i] = v;
}

extern "C" int pcl_cloud_pack_weights(const float* w, const int64_t* order, int64_t n, float* plane, int32_t* bad, void* stream)
{
    if (!w || !plane || !bad || n <= 0 || n > PCL_MAX_POINTS) return PCL_EINVAL;
    const int64_t stride = pcl_cloud_stride(n);
    hipLaunchKernelGGL(pcl_cloud_pack_weights_kernel, dim3((unsigned)(stride / PCL_BLOCK)), dim3(PCL_BLOCK), 0, (hipStream_t)stream, w, order, n,
                       stride, plane, bad);
    PCL_LAUNCH_CHECK();
    return 0;
}

__device__ inline uint64_t pcl_spread21(uint32_t v)
{
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_morton_kernel(const float* __restrict__ xyz, int64_t n, float lx, float ly,
                                                               float lz, float sx, float sy, float sz,
                                                               int64_t* __restrict__ keys)
{
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float top = 2097151.f;  // 2^21 - 1
    float fx = __builtin_amdgcn_fmed3f((xyz[3 * i] - lx) * sx, 0.f, top);
    float fy = __builtin_amdgcn_fmed3f((xyz[3 * i + 1] - ly) * sy, 0.f, top);
    float fz = __builtin_amdgcn_fmed3f((xyz[3 * i + 2] - lz) * sz, 0.f, top);
    uint64_t k = pcl_spread21((uint32_t)fx) | (pcl_spread21((uint32_t)fy) << 1) | (pcl_spread21((uint32_t)fz) << 2);
    keys[i] = (int64_t)k;
}

extern "C" int pcl_morton_keys(const float* xyz, int64_t n, const float* lo, const float* hi, int64_t* keys, void* stream)
{
    if (!xyz || !lo || !hi || !keys || n <= 0) return PCL_EINVAL;
    float s[3];
    for (int k = 0; k < 3; k++) s[k] = hi[k] > lo[k] ? 2097151.f / (hi[k] - lo[k]) : 0.f;
    hipLaunchKernelGGL(pcl_morton_kernel, dim3((unsigned)((n + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, xyz, n, lo[0], lo[1], lo[2], s[0], s[1], s[2], keys);
    PCL_LAUNCH_CHECK();
    return 0;
}

// ---- Morton order of a cloud, entirely on the device: bounding box -> 63-bit keys -> radix sort of (key, index) pairs.
__device__ __forceinline__ unsigned int pcl_ordered_key(float v)
{
    unsigned int b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pcl_ordered_value(unsigned int k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_bbox_kernel(const float* __restrict__ xyz, int64_t n, unsigned int* __restrict__ box)
{
    unsigned int lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PCL_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            unsigned int k = pcl_ordered_key(xyz[3 * i + c]);
            lo[c] = min(lo[c], k); hi[c] = max(hi[c], k);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = min(lo[c], (unsigned int)__shfl_xor((int)lo[c], o, 64));
            hi[c] = max(hi[c], (unsigned int)__shfl_xor((int)hi[c], o, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&box[c], lo[c]); atomicMax(&box[3 + c], hi[c]); }
    }
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_morton_box_kernel(const float* __restrict__ xyz, int64_t n, const unsigned int* __restrict__ box,
                                                                   unsigned long long* __restrict__ keys, int64_t* __restrict__ iota)
{
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float top = 2097151.f;  // 2^21 - 1
    unsigned long long k = 0ull;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float lo = pcl_ordered_value(box[c]), hi = pcl_ordered_value(box[3 + c]);
        float sc = hi > lo ? top / (hi - lo) : 0.f;
        float f = __builtin_amdgcn_fmed3f((xyz[3 * i + c] - lo) * sc, 0.f, top);
        k |= pcl_spread21((uint32_t)f) << c;
    }
    keys[i] = k;
    iota[i] = i;
}

static size_t order_sort_temp_bytes(int64_t n)
{
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs<rocprim::default_config, const unsigned long long*, unsigned long long*, const int64_t*, int64_t*>(
        nullptr, bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, 63, nullptr, false);
    return bytes;
}

// workspace of pcl_cloud_order: the bounding box (6 ordered-uint words in 64 bytes), the keys, the sorted keys, the identity permutation, the sort's temporary storage
struct OrderWs { unsigned int* box; unsigned long long *keys, *keys_sorted; int64_t* iota; void* temp; size_t temp_bytes; };
static size_t order_layout(void* base, int64_t n, OrderWs* w)
{
    if (n <= 0) return 0;
    PclCarve c{(char*)base, 0};
    w->box = (unsigned int*)c.take(64);
    w->keys = (unsigned long long*)c.take((size_t)n * 8);
    w->keys_sorted = (unsigned long long*)c.take((size_t)n * 8);
    w->iota = (int64_t*)c.take((size_t)n * 8);
    w->temp_bytes = order_sort_temp_bytes(n);
    w->temp = c.take(w->temp_bytes);
    return c.off;
}

extern "C" size_t pcl_cloud_order_workspace_bytes(int64_t n) { OrderWs w; return order_layout(nullptr, n, &w); }

// order[i] = index of the point that goes to packed slot i (Morton order of xyz inside its bounding box); feed it to
// pcl_cloud_pack.  Equal keys keep their original relative order (stable LSD radix sort).
extern "C" int pcl_cloud_order(const float* xyz, int64_t n, int64_t* order, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!xyz || !order || !workspace || n <= 0 || n > PCL_MAX_POINTS) return PCL_EINVAL;
    OrderWs w;
    if (workspace_bytes < order_layout(workspace, n, &w)) return PCL_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w.box, 0xff, 12, s);                          // lo = max key
    if (e == hipSuccess) e = hipMemsetAsync(w.box + 3, 0, 12, s);               // hi = min key
    if (e != hipSuccess) return (int)e;
    int64_t blocks = (n + PCL_BLOCK - 1) / PCL_BLOCK;
    hipLaunchKernelGGL(pcl_bbox_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(PCL_BLOCK), 0, s, xyz, n, w.box);
    hipLaunchKernelGGL(pcl_morton_box_kernel, dim3((unsigned)blocks), dim3(PCL_BLOCK), 0, s, xyz, n, w.box, w.keys, w.iota);
    PCL_LAUNCH_CHECK();
    e = rocprim::radix_sort_pairs(w.temp, w.temp_bytes, (const unsigned long long*)w.keys, w.keys_sorted, (const int64_t*)w.iota, order, (size_t)n, 0,
                                  63, s, false);
    return e == hipSuccess ? 0 : (int)e;
}

__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pack_kernel(const float* __restrict__ img, int H, int W,
                                                                  pcl_f4* __restrict__ pano)
{
    int Wp = W + 2, Hp = H + 2;
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= (int64_t)Wp * Hp) return;
    int yp = (int)(i / Wp), xp = (int)(i - (int64_t)yp * Wp);
    pcl_f4 v = {0.f, 0.f, 0.f, 0.f};
    if (yp >= 1 && yp <= H && xp >= 1 && xp <= W) {
        const float* s = img + ((int64_t)(yp - 1) * W + (xp - 1)) * 3;
        v.x = s[0]; v.y = s[1]; v.z = s[2];
    }
    pano[i] = v;
}

extern "C" int pcl_pano_pack(const float* img_hwc, int H, int W, float* pano, void* stream)
{
    if (!img_hwc || !pano || H <= 0 || W <= 0) return PCL_EINVAL;
    int64_t total = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(pcl_pano_pack_kernel, dim3((unsigned)((total + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, img_hwc, H, W, (pcl_f4*)pano);
    PCL_LAUNCH_CHECK();
    return 0;
}

// RGBA8 texels for images that are exactly k/255 (see include/piccolo_hip.h); flags anything else.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pack_u8_kernel(const float* __restrict__ img, int H, int W,
                                                                     uint32_t* __restrict__ pano, int* __restrict__ not_exact)
{
    int Wp = W + 2, Hp = H + 2;
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= (int64_t)Wp * Hp) return;
    int yp = (int)(i / Wp), xp = (int)(i - (int64_t)yp * Wp);
    uint32_t v = 0u;
    if (yp >= 1 && yp <= H && xp >= 1 && xp <= W) {
        const float* s = img + ((int64_t)(yp - 1) * W + (xp - 1)) * 3;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float f = s[c], k = rintf(f * 255.f);
            // uint8 -> .float() / 255. is an IEEE fp32 division: the value is exact iff dividing the level back gives f
            bad = bad || !(k >= 0.f && k <= 255.f) || __fdiv_rn(k, 255.f) != f;
            v |= ((uint32_t)k & 255u) << (8 * c);
        }
        if (bad) *not_exact = 1;
    }
    pano[i] = v;
}

// RGBA8 with the rows interleaved in pairs (PCL_PANO_U8P): the texel of bordered row yp, column xp goes to 32-bit word
// ((yp >> 1) * Wp + xp) * 2 + (yp & 1).  One thread per word of the padded layout (an odd H + 2 leaves a last half-pair: zeros).
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pack_u8p_kernel(const float* __restrict__ img, int H, int W,
                                                                      uint32_t* __restrict__ pano, int* __restrict__ not_exact)
{
    const int Wp = W + 2, pairs = (H + 3) >> 1;
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= (int64_t)Wp * pairs * 2) return;
    const int yp = (int)(i / Wp), xp = (int)(i - (int64_t)yp * Wp);
    uint32_t v = 0u;
    if (yp >= 1 && yp <= H && xp >= 1 && xp <= W) {
        const float* s = img + ((int64_t)(yp - 1) * W + (xp - 1)) * 3;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float f = s[c], k = rintf(f * 255.f);
            bad = bad || !(k >= 0.f && k <= 255.f) || __fdiv_rn(k, 255.f) != f;
            v |= ((uint32_t)k & 255u) << (8 * c);
        }
        if (bad) *not_exact = 1;
    }
    pano[((int64_t)(yp >> 1) * Wp + xp) * 2 + (yp & 1)] = v;
}

// RGBA8 in vertical pairs (PCL_PANO_U8V): element (xp, yp) = texel (xp, yp), texel (xp, yp + 1) of the bordered image.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pack_u8v_kernel(const float* __restrict__ img, int H, int W,
                                                                      pcl_i2* __restrict__ pano, int* __restrict__ not_exact)
{
    const int Wp = W + 2, Hp = H + 2;
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= (int64_t)Wp * Hp) return;
    const int yp = (int)(i / Wp), xp = (int)(i - (int64_t)yp * Wp);
    uint32_t v[2] = {0u, 0u};
    bool bad = false;
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const int y = yp + d;
        if (y >= 1 && y <= H && xp >= 1 && xp <= W) {
            const float* s = img + ((int64_t)(y - 1) * W + (xp - 1)) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float f = s[c], k = rintf(f * 255.f);
                bad = bad || !(k >= 0.f && k <= 255.f) || __fdiv_rn(k, 255.f) != f;
                v[d] |= ((uint32_t)k & 255u) << (8 * c);
            }
        }
    }
    if (bad) *not_exact = 1;
    pano[i] = (pcl_i2){(int)v[0], (int)v[1]};
}

extern "C" int pcl_pano_pack_u8v(const float* img_hwc, int H, int W, uint32_t* pano, int* not_exact, void* stream)
{
    if (!img_hwc || !pano || !not_exact || H <= 0 || W <= 0) return PCL_EINVAL;
    int64_t total = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(pcl_pano_pack_u8v_kernel, dim3((unsigned)((total + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, img_hwc, H, W, (pcl_i2*)pano, not_exact);
    PCL_LAUNCH_CHECK();
    return 0;
}

// half4 texels holding the levels 0..255 as fp16 (exact), for the same k/255 images as RGBA8.
__global__ void __launch_bounds__(PCL_BLOCK) pcl_pano_pack_f16_kernel(const float* __restrict__ img, int H, int W,
                                                                      pcl_i2* __restrict__ pano, int* __restrict__ not_exact)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    int Wp = W + 2, Hp = H + 2;
    int64_t i = (int64_t)blockIdx.x * PCL_BLOCK + threadIdx.x;
    if (i >= (int64_t)Wp * Hp) return;
    int yp = (int)(i / Wp), xp = (int)(i - (int64_t)yp * Wp);
    float lv[3] = {0.f, 0.f, 0.f};
    if (yp >= 1 && yp <= H && xp >= 1 && xp <= W) {
        const float* s = img + ((int64_t)(yp - 1) * W + (xp - 1)) * 3;
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float f = s[c], k = rintf(f * 255.f);
            bad = bad || !(k >= 0.f && k <= 255.f) || __fdiv_rn(k, 255.f) != f;
            lv[c] = k + 0.f;                                   // -0.0 is level 0: the +0 half, as the integer formats store it
        }
        if (bad) *not_exact = 1;
    }
    h2 rg = {(_Float16)lv[0], (_Float16)lv[1]}, b0 = {(_Float16)lv[2], (_Float16)0.f};
    pano[i] = (pcl_i2){__builtin_bit_cast(int, rg), __builtin_bit_cast(int, b0)};
}

extern "C" int pcl_pano_pack_f16(const float* img_hwc, int H, int W, void* pano, int* not_exact, void* stream)
{
    if (!img_hwc || !pano || !not_exact || H <= 0 || W <= 0) return PCL_EINVAL;
    int64_t total = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(pcl_pano_pack_f16_kernel, dim3((unsigned)((total + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, img_hwc, H, W, (pcl_i2*)pano, not_exact);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_pano_pack_u8p(const float* img_hwc, int H, int W, uint32_t* pano, int* not_exact, void* stream)
{
    if (!img_hwc || !pano || !not_exact || H <= 0 || W <= 0) return PCL_EINVAL;
    int64_t total = (int64_t)((H + 3) >> 1) * 2 * (W + 2);
    hipLaunchKernelGGL(pcl_pano_pack_u8p_kernel, dim3((unsigned)((total + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, img_hwc, H, W, pano, not_exact);
    PCL_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcl_pano_pack_u8(const float* img_hwc, int H, int W, uint32_t* pano, int* not_exact, void* stream)
{
    if (!img_hwc || !pano || !not_exact || H <= 0 || W <= 0) return PCL_EINVAL;
    int64_t total = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(pcl_pano_pack_u8_kernel, dim3((unsigned)((total + PCL_BLOCK - 1) / PCL_BLOCK)), dim3(PCL_BLOCK), 0,
                       (hipStream_t)stream, img_hwc, H, W, pano, not_exact);
    PCL_LAUNCH_CHECK();
    return 0;
}
