// pcl_host.h — host functions that one translation unit of the library defines and another calls (none of them is part of the C ABI),
// declared once, the carve helper behind every workspace layout, and the helpers that turn a runtime choice of kernel instance into a
// compile-time one.
#pragma once
#include <type_traits>

#include "pcl_device.h"

struct PclFuseArgs;      // pcl_gd_device.h
struct PclRoomTable;
struct PclDepthTable;

// ---- pcl_loss.hip: launch plans and the loss launches
// (sets > 1: the single-image plan of B / sets candidates for all B — pcl_plan_sets)
size_t pcl_partials_bytes(int64_t n, int B, int sets = 1);
int pcl_plan_nchunks(int64_t n, int B, int sets = 1);
int pcl_plan_nblocks(int64_t n, int B, int sets = 1);
int pcl_plan_G(int64_t n, int B, int sets = 1);
void pcl_plan_room_images(int64_t n, int per_image, int nimages, int* G, int* ngroups, int* nchunks, int* seg_len, int* steps_base, int* steps_rem);
void pcl_plan_for_groups(int64_t n, int ngroups, int* nchunks, int* seg_len, int* steps_base, int* steps_rem);
int pcl_launch_loss(const float* cloud, int64_t n, const void* pano, int pano_format, int H, int W, const PclPoseRec* poses, int B, bool grad,
                    const uint8_t* visible, float* partials, hipStream_t s, int flip, const PclFuseArgs* fuse, const PclDepthLook* depth,
                    int color_sets = 1, const float* weights = nullptr, int wsets = 0, int g0 = 0, int g1 = -1);
// a weighted launch runs the plan of (n, B) unchanged and has instances for one and two poses per block only (four exist through the
// experiments build's PCL_G): asked by the weighted entry points before they enqueue anything, and by pcl_launch_loss itself
static inline bool pcl_weighted_plan_ok(int64_t n, int B) { return n > 0 && n <= PCL_MAX_POINTS && B > 0 && pcl_plan_G(n, B) <= 2; }
int pcl_launch_loss_rooms(const PclRoomTable* rooms, const void* pano, int pano_format, int H, int W, const PclPoseRec* poses, int B, int G,
                          int ngroups, int nblk, float* partials, hipStream_t s, int flip, const PclFuseArgs* fuse, int color_sets = 1,
                          const PclDepthTable* dtab = nullptr, const PclDepthLook* depth = nullptr);

// ---- pcl_depth.hip: the z pass
size_t pcl_depth_zbuf_bytes(int B, int Hd, int Wd);
int pcl_depth_grid_check(int64_t n, int B, const PclDepthGrid& g);      // pcl_depth_check, for the entry points of pcl_depth_info.hip
int pcl_launch_zbuffers(const float* cloud, int64_t n, const PclPoseRec* poses, int B, const PclDepthGrid& g, int zstride, uint32_t* zbuf, bool fill,
                        hipStream_t s);

// Workspaces are carved in ONE place per family, a layout function that the size query runs without a base and the call with the
// caller's buffer: raw(bytes) is the next region as it comes (null without a base), take(bytes) one that ends on a 256-byte boundary;
// `off` is the size so far.
static inline size_t pcl_align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct PclCarve {
    char* base;
    size_t off;
    void* raw(size_t bytes) { void* p = base ? base + off : nullptr; off += bytes; return p; }
    void* take(size_t bytes) { return raw(pcl_align256(bytes)); }
};

// f(std::true_type{}) / f(std::false_type{}) for a runtime flag
template <class F>
static inline void pcl_with_flag(bool v, F&& f)
{
    if (v) return f(std::true_type{});
    f(std::false_type{});
}

// f(std::integral_constant<int, G>{}) for the runtime G: 4 where MAXG admits it, 2, else 1 — so that a kernel template with instances for
// G <= MAXG only (the rooms kernels: 1 and 2) gains none
template <int MAXG, class F>
static inline void pcl_with_G(int G, F&& f)
{
    if constexpr (MAXG >= 4) {
        if (G == 4) return f(std::integral_constant<int, 4>{});
    }
    if (G == 2) return f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 1>{});
}
