// space.hip -- haf_check_space (include/hafgrasp.h): the sample points of a fixed lattice inside the gripper's boxes, at each of n_grasps
// poses, classified against 1..8 depth views as UNSEEN, HIDDEN, FREE or HIT.  The per-sample rules are space_rules.h's, the same source
// haf_check_space_ref runs on the host: one fp32 transform per view, twelve rounded operations, then integers, so the two agree word
// for word (tests/test_space_gpu.py).
//
// One launch:
//   k_space_samples   grid (chunks of 256 samples, grasps), workgroups of 256: a lane owns ONE sample of ONE grasp.  19 grasps of the
//                     default lattice (4800 samples) are 361 workgroups, more than the chip has CUs; 4096 grasps at the cap are 2^20.
//                     The lattice, the views' constants and the pointers are the kernel's argument (scalar registers); the grasp's
//                     sixteen words are read at a workgroup-uniform address, scalar loads again.  A lane decodes its sample from the
//                     lattice (two 32-bit divisions for the indices, three 64-bit ones for the coordinates -- once per sample, not per
//                     view), forms its point in int64 and walks the views in a wave-uniform loop: transfer_project, ONE gather of a 2-
//                     or 4-byte depth sample at the projected pixel, the integer comparison.  A lane that has reached HIT sits the
//                     remaining views out (no later view can change a maximum that is already the largest rank) and a wave whose every
//                     lane has leaves the loop.  The gathers are scattered by nature; neighbouring samples fall on neighbouring pixels
//                     and the caches see that -- no image is staged in LDS.  Counts: one LDS integer atomic per sample into the
//                     workgroup's 16 counters, then at most 16 integer atomicAdds per workgroup on the grasp's zeroed row.  With
//                     `states` the lane also stores its byte.  A void grasp's workgroups write zero bytes and leave.
// No float atomics, no waiting between workgroups; the rows are integer sums, which do not depend on the order of arrival.
// Bounds: a lane works only for j < N; a pixel is read only where transfer_project reports TRANSFER_PROJECTS, which means 0 <= uc <
// width and 0 <= vc < height of that view; the LDS counters are indexed by region * 4 + state < 16; a grasp's words and row by
// blockIdx.y < n_grasps; a state byte at g * N + j < n_grasps * N.
#include "kernels.h"

namespace haf {

using namespace haf_space_math;

__global__ __launch_bounds__(kSpaceChunk) void k_space_samples(const SpaceDev d)
{
    __shared__ unsigned s_cnt[kSpaceRowWords];
    const unsigned g = blockIdx.y;
    const int N = d.l.first[SPACE_REGIONS];
    const int j = (int)(blockIdx.x * (unsigned)kSpaceChunk + threadIdx.x);       // (N <= 65536: no wrap)
    const bool live = j < N;
    const GraspWords gw = *reinterpret_cast<const GraspWords *>(d.grasps + (size_t)g * kClearGraspWords);      // (uniform)
    if (gw.reach_q < 0) {                                 // a void grasp (uniform over the workgroup)
        if (d.states && live) d.states[(size_t)g * (size_t)N + (size_t)j] = 0;
        return;
    }
    if (threadIdx.x < (unsigned)kSpaceRowWords) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (live) {
        int32_t stu[3], Pq[3];
        float p[3];
        const int region = space_sample(d.l, j, stu);
        space_point(gw, stu, Pq, p);
        int state = SPACE_UNSEEN;
        for (int k = 0; k < d.n_views; k++) {             // (k is wave-uniform: view k's constants are scalar loads)
            if (__ballot(state != SPACE_HIT) == 0) break;
            if (state == SPACE_HIT) continue;
            const SpaceViewRules &v = d.v[k];
            int32_t Qz, uc, vc, Zobs;
            if (transfer_project(v.r, p, Qz, uc, vc) != TRANSFER_PROJECTS) continue;
            const char *at = static_cast<const char *>(d.src[k]) + (size_t)vc * d.row_stride[k];
            const uint32_t raw = v.kind == HAF_FRAME_DEPTH_U16 ? (uint32_t)reinterpret_cast<const uint16_t *>(at)[uc]
                                                               : reinterpret_cast<const uint32_t *>(at)[uc];
            if (!space_observed(v, raw, Zobs)) continue;
            state = max(state, space_state(v.r, Qz, Zobs));
        }
        atomicAdd(&s_cnt[region * SPACE_STATES + state], 1u);
        if (d.states) d.states[(size_t)g * (size_t)N + (size_t)j] = (unsigned char)state;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)kSpaceRowWords) {
        const unsigned c = s_cnt[threadIdx.x];
        if (c) atomicAdd(d.rows + (size_t)g * kSpaceRowWords + threadIdx.x, c);
    }
}

void launch_space(const SpaceDev &d, hipStream_t s)
{
    const unsigned N = (unsigned)d.l.first[SPACE_REGIONS];
    if (N == 0) return;
    hipLaunchKernelGGL(k_space_samples, dim3((N + kSpaceChunk - 1) / kSpaceChunk, (unsigned)d.n_grasps), dim3(kSpaceChunk), 0, s, d);
}

}  // namespace haf
