// Translation unit of the episode-statistics reduction (lob_launch.h): episode_stats_partial_kernel / episode_stats_final_kernel.  A unit of
// its own, so that the units of the step and of lob_reset are compiled from what they were.  gfx950 only; no CPU execution path.
#define LOB_TU_SPLIT 1
#define LOB_TU_STATS 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"

int lobk_stats_chunks(int B) { return (B + LOB_STATS_CHUNK - 1) / LOB_STATS_CHUNK; }

void lobk_episode_stats(hipStream_t st, const StatsSrc& s, int n_groups, lob_episode_record* partial, lob_episode_record* out) {
    const int n_chunks = lobk_stats_chunks(s.B);
    hipLaunchKernelGGL(episode_stats_partial_kernel, dim3(n_chunks, n_groups), dim3(LOB_STATS_BLOCK), 0, st, s, n_chunks, partial);
    hipLaunchKernelGGL(episode_stats_final_kernel, dim3(n_groups), dim3(64), 0, st, partial, n_chunks, out);
}
