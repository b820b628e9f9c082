// pcl_gn_rooms.hip — the Levenberg-Marquardt polish of pcl_gn.hip for the winners of a rooms x images chain (additive to ABI 12; BUILD-DEFINED):
// pose (r, i) = row r * nimages + i against room r's cloud, panorama i and colour set i of room r, every room over its own chunking and its
// own region of partial rows.  The per-point pass is pcl_info_pass_at of pcl_info_device.h behind pcl_gn_pass_kernel's gate, the step is
// the text pcl_gn_step_kernel includes (pcl_gn_step_body.h), the chain is pcl_gn_chain of pcl_gn_device.h: record (r, i) has the bits of
// pcl_gn_refine of that pose, cloud, colour set and panorama alone.
#include <math.h>

#include "pcl_gn_device.h"

// The pass of pcl_gn_refine_rooms: pcl_pose_info_rooms_kernel's block behind the gate of its own pose (r, i); `state` is that of the launch's
// first image in room 0, rows r * btot + i apart like the poses read from it.
template <int FMT, bool CS>
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_pass_rooms_kernel(PclInfoArgs a, PclInfoImages im, PclInfoRooms rm, const PclGnState* __restrict__ state)
{
    const PclInfoRoomAt at = pcl_info_room_select(rm, (unsigned)a.pass.B);
    if (state[at.room * (unsigned)im.btot + at.image].frozen) return;      // (a scalar load: the address depends on the block alone)
    pcl_info_pass_rooms<FMT, CS>(a, im, at);
}

// The step of pcl_gn_refine_rooms: one block per pose (r, i) = blockIdx.x of B = nrooms * nimages, over room r's region and chunk count:
// pcl_gn_step_body.h, the one text of the step, with pose (r, i)'s rows being rows i of room r's [nchunks_r][nimages].
__global__ void __launch_bounds__(PCL_BLOCK) pcl_gn_step_rooms_kernel(const float* __restrict__ partials_all, PclInfoRooms rm, int nimages, int B,
                                                                     PclGnState* __restrict__ state, pcl_gn_hyper hp, int k, int iters,
                                                                     float* __restrict__ out, float* __restrict__ info, float* __restrict__ cov,
                                                                     float* __restrict__ trace)
{
    const int b = blockIdx.x, room = b / nimages, rowsB = nimages, row = b - room * nimages;
    const float* __restrict__ partials = partials_all + rm.rec[room].rows;
    const int nchunks = rm.rec[room].nchunks;
#include "pcl_gn_step_body.h"
}

extern "C" size_t pcl_gn_rooms_workspace_bytes(const pcl_gd_room* rooms_host, int nrooms, int nimages)
{
    PclInfoRoomsPlan g;
    return pcl_info_rooms_plan(rooms_host, nrooms, nimages, &g) ? 0 : g.bytes;
}

// pcl_gn_refine for the nrooms * nimages poses (r, i), each against room r's cloud, colour set i and panos_host[i], in one chain: the init
// launch runs over all poses as it is, the gated rooms pass once per PCL_RES_MAX_IMAGES images over all rooms, the rooms step over all
// poses.  1 + (groups + 1) (iters + 1) launches.
extern "C" int pcl_gn_refine_rooms(const pcl_gd_room* rooms_host, int nrooms, int color_sets, const uint64_t* panos_host, int nimages, int pano_format,
                                   int H, int W, const float* trans, const float* rot, int pose_stride, const pcl_gn_hyper* hyper_host, int iters,
                                   void* state, float* out, float* info, float* cov, float* trace, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pcl_gn_entry_ok(hyper_host, iters, state, out, info, workspace)) return PCL_EINVAL;
    PclInfoArgs a;
    PclInfoImages im;
    PclInfoRoomsPlan g;
    const int rc = pcl_info_rooms_args(&a, &im, &g, rooms_host, nrooms, color_sets, panos_host, nimages, pano_format, H, W, trans, rot, pose_stride);
    if (rc) return rc;
    if (workspace_bytes < g.bytes) return PCL_EINVAL;
    const int B = nrooms * nimages;
    const dim3 blk(PCL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    return pcl_gn_chain(
        a, B, hyper_host, iters, state, trace, workspace, s,
        [&](const PclInfoArgs& ak, const PclGnState* st) {
            pcl_info_rooms_launches(ak, im, g, panos_host, [&](const PclInfoArgs& al, const PclInfoImages& il, const PclInfoRooms& tl, int i0, dim3 grid) {
                pcl_with_flag(color_sets > 1, [&](auto cs) {
                    pcl_with_pass_fmt(pano_format, [&](auto fmt) {
                        hipLaunchKernelGGL((pcl_gn_pass_rooms_kernel<decltype(fmt)::value, decltype(cs)::value>), grid, blk, 0, s, al, il, tl, st + i0);
                    });
                });
            });
            return 0;
        },
        [&](const float* partials, PclGnState* st, const pcl_gn_hyper& hp, int k) {
            hipLaunchKernelGGL(pcl_gn_step_rooms_kernel, dim3((unsigned)B), blk, 0, s, partials, g.t, nimages, B, st, hp, k, iters, out, info, cov, trace);
            PCL_LAUNCH_CHECK();
            return 0;
        });
}
