// Host-side argument checking of pcl_pose_information_images and pcl_gn_refine_images under AddressSanitizer and UBSan: a stand-alone
// program linked against the host code of csrc/pcl_info.hip and csrc/pcl_gn.hip.  Every call below must answer PCL_EINVAL (-1) before any
// launch, so it runs on a machine without a GPU; the panorama list is a real host array (the checks read it, up to 70 entries).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined piccolo_amd/csrc/pcl_info.hip \
//         piccolo_amd/csrc/pcl_gn.hip piccolo_amd/csrc/pcl_pack.hip tools/host_checks/gn_images_refusals.cpp -o gn_images_refusals \
//         && ./gn_images_refusals
// (pcl_pack.hip: pcl_cloud_stride and pcl_cloud_sets_bytes, which the shared argument check calls)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/piccolo_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                        \
    do {                                                                          \
        const long long got_ = (long long)(what);                                 \
        if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #what, got_, (long long)(want)); failures++; } \
    } while (0)

struct Args {
    const float *cloud, *weights;
    int wsets;
    int64_t n;
    int csets;
    std::vector<uint64_t> panos;
    bool null_panos;
    int I, fmt, H, W;
    const float *trans, *rot;
    int stride;
    pcl_gn_hyper hyper;
    int iters;
    void* state;
    float *out, *info, *cov, *trace;
    void* work;
    size_t nbytes;
};

static int info_call(const Args& a)
{
    return pcl_pose_information_images(a.cloud, a.weights, a.wsets, a.n, a.csets, a.null_panos ? nullptr : a.panos.data(), a.I, a.fmt, a.H, a.W, a.trans,
                                       a.rot, a.stride, a.info, a.cov, a.work, a.nbytes, nullptr);
}

static int gn_call(const Args& a)
{
    return pcl_gn_refine_images(a.cloud, a.weights, a.wsets, a.n, a.csets, a.null_panos ? nullptr : a.panos.data(), a.I, a.fmt, a.H, a.W, a.trans, a.rot,
                                a.stride, &a.hyper, a.iters, a.state, a.out, a.info, a.cov, a.trace, a.work, a.nbytes, nullptr);
}

static std::vector<uint64_t> list(int I, int hole = -1)
{
    std::vector<uint64_t> v;
    for (int i = 0; i < I; i++) v.push_back(i == hole ? 0 : 0x900000ull + 0x1000ull * i);
    return v;
}

int main()
{
    float* const p = (float*)0x10000;      // never dereferenced on the host
    const Args good = {p, nullptr, 0, 1025, 1, list(3), false, 3, 2, 32, 64, p, p, 3, {1e-3f, 10.f, 0.1f, 1e-9f, 1e9f, 0.1f, 0.f}, 5, p, p, p, p, p, p,
                       pcl_gn_workspace_bytes(1025, 3)};
    EXPECT(good.nbytes > 0, 1); EXPECT(good.nbytes, pcl_pose_information_workspace_bytes(1025, 3));
    Args a;
#define REFUSED(change) do { a = good; change; EXPECT(info_call(a), -1); EXPECT(gn_call(a), -1); } while (0)
    REFUSED(a.cloud = nullptr); REFUSED(a.trans = nullptr); REFUSED(a.rot = nullptr); REFUSED(a.info = nullptr); REFUSED(a.work = nullptr);
    REFUSED(a.null_panos = true);
    for (int hole = 0; hole < 3; hole++) REFUSED(a.panos = list(3, hole));
    REFUSED((a.I = 70, a.panos = list(70, 69), a.nbytes = (size_t)1 << 30)); REFUSED((a.I = 70, a.panos = list(70, 64), a.nbytes = (size_t)1 << 30));
    REFUSED(a.I = 0); REFUSED(a.I = -3);
    REFUSED(a.wsets = 1); REFUSED(a.wsets = 3);                 // no weights: 0 only
    REFUSED((a.weights = p, a.wsets = 0)); REFUSED((a.weights = p, a.wsets = 2)); REFUSED((a.weights = p, a.wsets = 4)); REFUSED((a.weights = p, a.wsets = -1));
    REFUSED(a.csets = -1); REFUSED(a.csets = 2); REFUSED(a.csets = 4);
    // one buffer resource each: 2^24 points are 64 MiB a plane
    REFUSED((a.n = (int64_t)1 << 24, a.I = 32, a.panos = list(32), a.weights = p, a.wsets = 32, a.nbytes = (size_t)1 << 40));
    REFUSED((a.n = (int64_t)1 << 24, a.I = 10, a.panos = list(10), a.csets = 10, a.nbytes = (size_t)1 << 40));
    REFUSED(a.n = 0); REFUSED(a.n = -1); REFUSED((a.n = ((int64_t)1 << 27) + 1, a.nbytes = (size_t)1 << 40));
    REFUSED(a.H = 0); REFUSED(a.W = -1); REFUSED(a.fmt = 3); REFUSED(a.fmt = 4); REFUSED(a.fmt = -1);
    REFUSED(a.stride = 2); REFUSED(a.stride = 0); REFUSED(a.stride = -16);
    REFUSED((a.fmt = 0, a.H = 1 << 14, a.W = 1 << 13));
    REFUSED(a.nbytes = good.nbytes - 1); REFUSED(a.nbytes = 0); REFUSED((a.I = 4, a.panos = list(4)));
#undef REFUSED
#define REFUSED(change) do { a = good; change; EXPECT(gn_call(a), -1); } while (0)
    REFUSED(a.iters = -1); REFUSED(a.iters = 1001); REFUSED(a.state = nullptr); REFUSED(a.out = nullptr);
    REFUSED(a.hyper.lam0 = 0.f); REFUSED(a.hyper.lam_up = 1.f); REFUSED(a.hyper.lam_down = 1.5f); REFUSED((a.hyper.lam_min = 2.f, a.hyper.lam_max = 1.f));
    REFUSED(a.hyper.step_cap = 0.f); REFUSED(a.hyper.tol = -1e-9f);
    std::printf(failures ? "%d refusals missing\n" : "every refusal answered PCL_EINVAL\n", failures);
    return failures ? 1 : 0;
}
