// pcl_prune.hip — pcl_gd_prune: keep the best candidates of every group of a GD state and hand their complete optimiser state to a
// smaller state, on the device (no host round trip, capture-safe).  One 256-thread block per group, one launch, no workspace, no atomics.
#include "pcl_gd_state.h"

#define PCL_PRUNE_THREADS 256
#define PCL_PRUNE_WAVES (PCL_PRUNE_THREADS / PCL_WAVE)
// 16-byte words a survivor moves: its PclGdPose, its pose record of copy 0, its pose record of copy 1 (the shadow: panorama and colour set)
#define PCL_PRUNE_POSE_V4 ((int)(sizeof(PclGdPose) / 16))
#define PCL_PRUNE_REC_V4 ((int)(sizeof(PclPoseRec) / 16))
#define PCL_PRUNE_V4 (PCL_PRUNE_POSE_V4 + 2 * PCL_PRUNE_REC_V4)
static_assert(sizeof(PclGdPose) % 16 == 0 && sizeof(PclPoseRec) % 16 == 0, "records move as 16-byte words");

// Block g: the group's last losses into LDS, every thread ranks its candidates by counting those ahead of them (pcl_gd_better is a
// strict total order, so the rank is the step at which `keep` successive "take the winner, remove it" steps would take the candidate),
// survivors get their slots in ORIGINAL index order — wave64 ballot / popcount prefix, the waves' counts scanned through LDS, 256
// candidates per round —, then the lanes move the survivors' records as 16-byte words.
__global__ void __launch_bounds__(PCL_PRUNE_THREADS) pcl_gd_prune_kernel(const PclGdPose* __restrict__ st_in, const PclPoseRec* __restrict__ recs_in0,
                                                                         const PclPoseRec* __restrict__ recs_in1, int per_group, int keep,
                                                                         PclGdPose* __restrict__ st_out, PclPoseRec* __restrict__ recs_out0,
                                                                         PclPoseRec* __restrict__ recs_out1, int32_t* __restrict__ survivors,
                                                                         float* __restrict__ leaf_trans, float* __restrict__ leaf_rot)
{
    __shared__ float loss_sh[PCL_GD_PRUNE_MAX];
    __shared__ int src_sh[PCL_GD_PRUNE_MAX];            // survivor slot -> index inside the group
    __shared__ int count_sh[PCL_PRUNE_WAVES];
    const int tid = threadIdx.x, lane = tid & (PCL_WAVE - 1), wave = tid / PCL_WAVE;
    const int64_t in0 = (int64_t)blockIdx.x * per_group, out0 = (int64_t)blockIdx.x * keep;
    const PclGdPose* s = st_in + in0;
    for (int b = tid; b < per_group; b += PCL_PRUNE_THREADS) loss_sh[b] = s[b].last_loss;
    __syncthreads();

    int base = 0;                                       // survivors of the earlier rounds (the same in every thread)
    for (int b0 = 0; b0 < per_group; b0 += PCL_PRUNE_THREADS) {
        const int b = b0 + tid;
        bool kept = false;
        if (b < per_group) {
            const float l = loss_sh[b];
            int ahead = 0;
            for (int j = 0; j < per_group; j++) ahead += pcl_gd_better(loss_sh[j], j, l, b) ? 1 : 0;
            kept = ahead < keep;
        }
        const unsigned long long mask = __ballot(kept);
        if (lane == 0) count_sh[wave] = __popcll(mask);
        __syncthreads();
        int slot = base + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < PCL_PRUNE_WAVES; w++) {
            const int c = count_sh[w];
            if (w < wave) slot += c;
            total += c;
        }
        if (kept) src_sh[slot] = b;                     // (slot < keep: exactly `keep` candidates have fewer than `keep` ahead of them)
        base += total;
        __syncthreads();
    }

    for (int q = tid; q < keep * PCL_PRUNE_V4; q += PCL_PRUNE_THREADS) {
        const int slot = q / PCL_PRUNE_V4, w = q - slot * PCL_PRUNE_V4;
        const int64_t src = in0 + src_sh[slot], dst = out0 + slot;
        if (w < PCL_PRUNE_POSE_V4) ((pcl_f4*)(st_out + dst))[w] = ((const pcl_f4*)(st_in + src))[w];
        else if (w < PCL_PRUNE_POSE_V4 + PCL_PRUNE_REC_V4) ((pcl_f4*)(recs_out0 + dst))[w - PCL_PRUNE_POSE_V4] = ((const pcl_f4*)(recs_in0 + src))[w - PCL_PRUNE_POSE_V4];
        else ((pcl_f4*)(recs_out1 + dst))[w - PCL_PRUNE_POSE_V4 - PCL_PRUNE_REC_V4] = ((const pcl_f4*)(recs_in1 + src))[w - PCL_PRUNE_POSE_V4 - PCL_PRUNE_REC_V4];
    }
    for (int slot = tid; slot < keep; slot += PCL_PRUNE_THREADS) survivors[out0 + slot] = src_sh[slot];
    // every INPUT candidate's leaf parameters, as pcl_gd_winner hands them back
    for (int b = tid; b < per_group; b += PCL_PRUNE_THREADS) {
        const int64_t row = (in0 + b) * 3;
        for (int q = 0; q < 3; q++) {
            if (leaf_trans) leaf_trans[row + q] = s[b].leaf[q];
            if (leaf_rot) leaf_rot[row + q] = s[b].leaf[3 + q];
        }
    }
}

extern "C" int pcl_gd_prune(const void* state_in, int groups, int per_group, int keep, void* state_out, int32_t* survivors, float* leaf_trans,
                            float* leaf_rot, void* stream)
{
    if (!state_in || !state_out || !survivors || state_out == state_in) return PCL_EINVAL;
    if (groups <= 0 || keep <= 0 || keep > per_group || per_group > PCL_GD_PRUNE_MAX) return PCL_EINVAL;
    if ((int64_t)groups * per_group > 0x7fffffff / 2) return PCL_EINVAL;
    if (((uintptr_t)state_in | (uintptr_t)state_out) & 15) return PCL_EINVAL;      // (the records move as 16-byte words)
    const int Bin = groups * per_group, Bout = groups * keep;
    void* in = const_cast<void*>(state_in);
    hipLaunchKernelGGL(pcl_gd_prune_kernel, dim3(groups), dim3(PCL_PRUNE_THREADS), 0, (hipStream_t)stream, gd_poses(in, Bin), gd_recs(in, Bin, 0),
                       gd_recs(in, Bin, 1), per_group, keep, gd_poses(state_out, Bout), gd_recs(state_out, Bout, 0), gd_recs(state_out, Bout, 1), survivors,
                       leaf_trans, leaf_rot);
    PCL_LAUNCH_CHECK();
    return 0;
}
