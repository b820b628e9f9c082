// pcl_timer.h — the kernel timer's host-side pool of event pairs (pcl_timer_* of include/piccolo_hip.h, pcl_timer.hip) and the two calls
// with which a GD iteration loop brackets its loss launch.
#pragma once
#include <hip/hip_runtime.h>

struct PclTimer {
    int capacity, used, stride;
    hipEvent_t* start;
    hipEvent_t* stop;
};

// Before the loss launch of iteration `it`.  Every `stride`-th iteration only, and while slots remain: an event pair costs a few
// microseconds of GPU timeline, which would distort short kernels if it bracketed all of them.  *timed: pcl_timer_end has to follow.
static inline hipError_t pcl_timer_begin(PclTimer* t, int it, hipStream_t s, bool* timed)
{
    *timed = t && t->used < t->capacity && (it % t->stride) == 0;
    return *timed ? hipEventRecord(t->start[t->used], s) : hipSuccess;
}

// After it.  Only a completed start / stop pair counts as used: pcl_timer_read never sees a half-recorded slot.
static inline hipError_t pcl_timer_end(PclTimer* t, hipStream_t s)
{
    const hipError_t e = hipEventRecord(t->stop[t->used], s);
    if (e == hipSuccess) t->used++;
    return e;
}
