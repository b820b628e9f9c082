// pcl_gn_device.h — what pcl_gn.hip, pcl_gn_rooms.hip and pcl_depth_info.hip share of the Levenberg-Marquardt chain: the per-pose state, the
// entry check of every pcl_gn_refine* call, the init and step launches and the chain driver, whose pass and step callbacks return an
// error code that ends the chain.  The step kernels' body, the other thing they share, is the text
// pcl_gn_step_body.h.  The rooms chain is a translation unit of its own: a second step kernel beside pcl_gn_step_kernel changes how the
// compiler inlines the double-precision library calls of both, and pcl_gn_step_kernel keeps the instruction stream it had.
#pragma once
#include <math.h>

#include "pcl_info_device.h"

#define PCL_GN_OUT 16                      // floats per out / trace row (include/piccolo_hip.h)
#define PCL_GN_MAX_ITERS 1000

// Per pose, in the caller's state buffer.  The pass reads theta_try in place: trans = &tri[0], rot = &tri[3], pose stride sizeof / 4.
struct PclGnState {
    double H[6][6], b[6], M, S1, S2;       // the accepted evaluation's sums (k = 0 refused: the refused ones)
    float acc[6];                          // theta_acc: t, yaw, pitch, roll
    float tri[6];                          // theta_try
    float F_acc, F_start, lam;
    int accepted, rejected, evaluations, status, frozen, sums_ok, pad;
};
static_assert(sizeof(PclGnState) % 8 == 0, "state rows keep their doubles aligned");

static inline bool pcl_gn_hyper_ok(const pcl_gn_hyper* h)
{
    const float v[7] = {h->lam0, h->lam_up, h->lam_down, h->lam_min, h->lam_max, h->step_cap, h->tol};
    for (int i = 0; i < 7; i++)
        if (!(fabsf(v[i]) <= 3.402823466e38f)) return false;
    return h->lam0 > 0.f && h->lam_up > 1.f && h->lam_down > 0.f && h->lam_down <= 1.f && h->lam_min <= h->lam_max && h->step_cap > 0.f && h->tol >= 0.f;
}

// What every pcl_gn_refine* entry point checks first, before its form's own arguments: the buffers it cannot do without, iters, the hyper
static inline bool pcl_gn_entry_ok(const pcl_gn_hyper* hyper_host, int iters, const void* state, const float* out, const float* info, const void* workspace)
{
    if (!hyper_host || !state || !out || !info || !workspace) return false;
    return iters >= 0 && iters <= PCL_GN_MAX_ITERS && pcl_gn_hyper_ok(hyper_host);
}

// pcl_gn_init_kernel over B poses (pcl_gn.hip)
int pcl_gn_launch_init(PclGnState* state, const float* trans, const float* rot, int pose_stride, float lam0, float* trace, int B, int iters, hipStream_t s);
// pcl_gn_step_kernel over B poses (pcl_gn.hip): the one place that launches it, for the chains of pcl_gn.hip and of pcl_depth_info.hip
int pcl_gn_launch_step(const float* partials, int nchunks, int B, PclGnState* state, const pcl_gn_hyper& hp, int k, int iters, float* out, float* info,
                       float* cov, float* trace, hipStream_t s);

// The chain of all three forms over B poses: `a` comes from the form's argument check with the caller's poses in a.pass.  The init launch
// reads them; from then on the state is the pose source (theta_try in place) and the workspace holds the partial rows.  Evaluation
// k = 0 .. iters is pass(a, st), whatever launches the form's gated pass takes, and step(a.partials, st, hp, k), its one step launch.
// Both return 0 or an error code; the chain returns the first one that is not 0, or a launch error, at once and enqueues nothing after it.
template <class Pass, class Step>
static inline int pcl_gn_chain(PclInfoArgs& a, int B, const pcl_gn_hyper* hyper_host, int iters, void* state, float* trace, void* workspace, hipStream_t s,
                               Pass&& pass, Step&& step)
{
    PclGnState* st = (PclGnState*)state;
    const pcl_gn_hyper hp = *hyper_host;
    int rc = pcl_gn_launch_init(st, a.pass.trans, a.pass.rot, a.pass.pose_stride, hp.lam0, trace, B, iters, s);
    if (rc) return rc;
    a.partials = (float*)workspace;
    a.pass.trans = st->tri; a.pass.rot = st->tri + 3; a.pass.pose_stride = (int)(sizeof(PclGnState) / sizeof(float));
    for (int k = 0; k <= iters; k++) {
        rc = pass(a, (const PclGnState*)st);
        if (rc) return rc;
        PCL_LAUNCH_CHECK();
        rc = step((const float*)a.partials, st, hp, k);
        if (rc) return rc;
    }
    return 0;
}
