// pcl_gd_state.h — the GD state blob's layout and the order of its candidates, shared by pcl_gd.hip (runs, pcl_gd_winner) and
// pcl_prune.hip (pcl_gd_prune).
#pragma once
#include "pcl_device.h"

// state blob = { PclGdPose[B], PclPoseRec[B] } x 2: copy 0 is the canonical one (what pcl_gd_init fills and pcl_gd_result reads);
// fused iterations ping-pong between the two (a block of iteration k + 1 reads iteration k's copy while the block of chunk 0
// writes iteration k + 1's).  The panorama addresses of the pose records are kept in both copies.
static inline size_t gd_copy_bytes(int B) { return (size_t)B * (sizeof(PclGdPose) + sizeof(PclPoseRec)); }
static inline PclGdPose* gd_poses(void* state, int B = 0, int copy = 0) { return (PclGdPose*)((char*)state + (size_t)copy * gd_copy_bytes(B)); }
static inline PclPoseRec* gd_recs(void* state, int B, int copy = 0)
{
    return (PclPoseRec*)((char*)state + (size_t)copy * gd_copy_bytes(B) + (size_t)B * sizeof(PclGdPose));
}

#define PCL_GD_NO_CANDIDATE 0x7fffffff

// Is candidate ia with last loss la ahead of candidate ib with lb?  torch.argmin's rules (omniloc.py:271): a NaN beats any number, among
// equals — or among NaNs — the smaller index wins (-0.0 == +0.0); index PCL_GD_NO_CANDIDATE is behind every candidate.  A strict total
// order of the candidates of a group.
__device__ __forceinline__ bool pcl_gd_better(float la, int ia, float lb, int ib)
{
    if (ib == PCL_GD_NO_CANDIDATE) return ia != PCL_GD_NO_CANDIDATE;
    if (ia == PCL_GD_NO_CANDIDATE) return false;
    const bool na = la != la, nb = lb != lb;
    if (na != nb) return na;
    if (na || la == lb) return ia < ib;
    return la < lb;
}
