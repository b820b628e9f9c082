// pcl_timer.hip — the kernel timer of the C ABI (include/piccolo_hip.h): a pool of event pairs that the GD iteration loops record
// around their loss launches (pcl_timer.h) and pcl_timer_read adds up.  Host code only.
#include "pcl_timer.h"

#include "../../include/piccolo_hip.h"

extern "C" void* pcl_timer_create(int capacity)
{
    if (capacity <= 0) return nullptr;
    PclTimer* t = new PclTimer;
    t->capacity = capacity; t->used = 0; t->stride = 1;
    t->start = new hipEvent_t[capacity];
    t->stop = new hipEvent_t[capacity];
    for (int i = 0; i < capacity; i++) {
        if (hipEventCreate(&t->start[i]) != hipSuccess || hipEventCreate(&t->stop[i]) != hipSuccess) {
            for (int j = 0; j <= i; j++) { (void)hipEventDestroy(t->start[j]); if (j < i) (void)hipEventDestroy(t->stop[j]); }
            delete[] t->start; delete[] t->stop; delete t;
            return nullptr;
        }
    }
    return t;
}

extern "C" void pcl_timer_destroy(void* timer)
{
    PclTimer* t = (PclTimer*)timer;
    if (!t) return;
    for (int i = 0; i < t->capacity; i++) { (void)hipEventDestroy(t->start[i]); (void)hipEventDestroy(t->stop[i]); }
    delete[] t->start; delete[] t->stop; delete t;
}

extern "C" void pcl_timer_reset(void* timer) { if (timer) ((PclTimer*)timer)->used = 0; }

extern "C" void pcl_timer_set_stride(void* timer, int stride) { if (timer && stride > 0) ((PclTimer*)timer)->stride = stride; }

extern "C" int pcl_timer_read(void* timer, double* total_ms_host, int* launches_host)
{
    PclTimer* t = (PclTimer*)timer;
    if (!t || !total_ms_host || !launches_host) return PCL_EINVAL;
    double total = 0.0;
    for (int i = 0; i < t->used; i++) {
        hipError_t e = hipEventSynchronize(t->stop[i]);
        if (e != hipSuccess) return (int)e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, t->start[i], t->stop[i]);
        if (e != hipSuccess) return (int)e;
        total += (double)ms;
    }
    *total_ms_host = total; *launches_host = t->used;
    return 0;
}

extern "C" int pcl_timer_calibrate(void* timer, int reps, double* pair_ms_host, void* stream)
{
    if (!timer || !pair_ms_host || reps <= 0 || reps > 4096) return PCL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t a, b;
    hipError_t e = hipEventCreate(&a);
    if (e != hipSuccess) return (int)e;
    e = hipEventCreate(&b);
    if (e != hipSuccess) { (void)hipEventDestroy(a); return (int)e; }
    float* ms = new float[reps];
    int got = 0;
    for (int i = 0; i < reps && e == hipSuccess; i++) {
        e = hipEventRecord(a, s);
        if (e == hipSuccess) e = hipEventRecord(b, s);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[got], a, b);
        if (e == hipSuccess) got++;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    if (e == hipSuccess) {
        for (int i = 1; i < got; i++) {                      // insertion sort: a few dozen values
            float v = ms[i]; int j = i - 1;
            while (j >= 0 && ms[j] > v) { ms[j + 1] = ms[j]; j--; }
            ms[j + 1] = v;
        }
        *pair_ms_host = (double)ms[got / 2];
    }
    delete[] ms;
    return (int)e;
}
