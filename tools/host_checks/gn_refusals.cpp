// Host-side argument checking of pcl_gn_refine under AddressSanitizer and UBSan: a stand-alone program linked against the host code of
// csrc/pcl_gn.hip.  Every call below must answer PCL_EINVAL (-1) before any HIP call, so it runs on a machine without a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         piccolo_amd/csrc/pcl_gn.hip piccolo_amd/csrc/pcl_pack.hip tools/host_checks/gn_refusals.cpp -o gn_refusals && ./gn_refusals
// (pcl_pack.hip: pcl_cloud_stride, which the shared argument check calls)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../include/piccolo_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                        \
    do {                                                                          \
        const long long got_ = (long long)(what);                                 \
        if (got_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #what, got_, (long long)(want)); failures++; } \
    } while (0)

struct Args {
    const float *cloud, *weights;
    int64_t n;
    const void* pano;
    int fmt, H, W;
    const float *trans, *rot;
    int stride, B;
    pcl_gn_hyper hyper;
    bool null_hyper;
    int iters;
    void* state;
    float *out, *info, *cov, *trace;
    void* work;
    size_t nbytes;
};

static int call(const Args& a)
{
    return pcl_gn_refine(a.cloud, a.weights, a.n, a.pano, a.fmt, a.H, a.W, a.trans, a.rot, a.stride, a.B, a.null_hyper ? nullptr : &a.hyper, a.iters,
                         a.state, a.out, a.info, a.cov, a.trace, a.work, a.nbytes, nullptr);
}

int main()
{
    // addresses that are never dereferenced on the host
    float* const p = (float*)0x10000;
    const Args good = {p, nullptr, 1025, p, 2, 32, 64, p, p, 3, 3, {1e-3f, 10.f, 0.1f, 1e-9f, 1e9f, 0.1f, 0.f}, false, 5, p, p, p, p, p, p,
                       pcl_gn_workspace_bytes(1025, 3)};
    EXPECT(pcl_gn_state_bytes(0), 0); EXPECT(pcl_gn_state_bytes(-7), 0); EXPECT(pcl_gn_state_bytes(3) > 0, 1);
    EXPECT(pcl_gn_workspace_bytes(0, 1), 0); EXPECT(pcl_gn_workspace_bytes(1025, 0), 0); EXPECT(pcl_gn_workspace_bytes(((int64_t)1 << 27) + 1, 1), 0);
    EXPECT(pcl_gn_workspace_bytes((int64_t)1 << 27, 1 << 22), 0); EXPECT(good.nbytes > 0, 1);
    Args a;
#define REFUSED(change) do { a = good; change; EXPECT(call(a), -1); } while (0)
    REFUSED(a.cloud = nullptr); REFUSED(a.pano = nullptr); REFUSED(a.trans = nullptr); REFUSED(a.rot = nullptr); REFUSED(a.info = nullptr);
    REFUSED(a.work = nullptr); REFUSED(a.null_hyper = true); REFUSED(a.state = nullptr); REFUSED(a.out = nullptr);
    REFUSED(a.n = 0); REFUSED(a.n = -1); REFUSED((a.n = ((int64_t)1 << 27) + 1, a.nbytes = (size_t)1 << 40));
    REFUSED(a.B = 0); REFUSED(a.B = -2); REFUSED(a.B = 4); REFUSED((a.n = (int64_t)1 << 27, a.B = 1 << 22, a.nbytes = (size_t)1 << 60));
    REFUSED(a.H = 0); REFUSED(a.W = -1); REFUSED(a.fmt = 3); REFUSED(a.fmt = 4); REFUSED(a.fmt = 7); REFUSED(a.fmt = -1);
    REFUSED(a.stride = 2); REFUSED(a.stride = 0); REFUSED(a.stride = -16);
    REFUSED((a.fmt = 0, a.H = 1 << 14, a.W = 1 << 13));
    REFUSED(a.nbytes = good.nbytes - 1); REFUSED(a.nbytes = 0);
    REFUSED(a.iters = -1); REFUSED(a.iters = 1001); REFUSED(a.iters = std::numeric_limits<int>::min()); REFUSED(a.iters = std::numeric_limits<int>::max());
    const float bad[3] = {std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (float v : bad) {
        REFUSED(a.hyper.lam0 = v); REFUSED(a.hyper.lam_up = v); REFUSED(a.hyper.lam_down = v); REFUSED(a.hyper.lam_min = v);
        REFUSED(a.hyper.lam_max = v); REFUSED(a.hyper.step_cap = v); REFUSED(a.hyper.tol = v);
    }
    REFUSED(a.hyper.lam0 = 0.f); REFUSED(a.hyper.lam0 = -1e-3f); REFUSED(a.hyper.lam_up = 1.f); REFUSED(a.hyper.lam_up = 0.5f);
    REFUSED(a.hyper.lam_down = 0.f); REFUSED(a.hyper.lam_down = -0.1f); REFUSED(a.hyper.lam_down = 1.5f);
    REFUSED((a.hyper.lam_min = 2.f, a.hyper.lam_max = 1.f)); REFUSED(a.hyper.step_cap = 0.f); REFUSED(a.hyper.step_cap = -0.1f);
    REFUSED(a.hyper.tol = -1e-9f);
    std::printf(failures ? "%d refusals missing\n" : "every refusal answered PCL_EINVAL\n", failures);
    return failures ? 1 : 0;
}
