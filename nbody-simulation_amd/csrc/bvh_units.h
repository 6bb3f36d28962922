// What the units of the device-side BVH build (f32) offer bvh_build.hip on the host: one launcher per launch site of
// bvh_build_levels and bvh_build_finish.  Each holds its kernel's <<<grid, block, 0, s>>> and nothing else (the scratch
// pointers are an internal type of each unit, so a launcher takes the scratch and its layout); the caller asks
// hipGetLastError.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_build.h"

namespace nbody {

// bvh_fold.hip: the chain of a level's long nodes.  gc: work-groups of the passes over chunks, gb: long nodes of the level
void launch_bvh_chunk_sums(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level);
void launch_bvh_chunk_runs(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level);
void launch_bvh_big_fold(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gb, int level, int use_runs);

// bvh_partition.hip: counts, split and children of a level's long nodes, then the swaps
void launch_bvh_big_count(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level, int leaf_size);
void launch_bvh_big_ranks(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level);
void launch_bvh_big_ranks_lists(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level);
void launch_bvh_big_swap(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gc, int level);

// bvh_subtrees.hip.  gs: work-groups
void launch_bvh_subtrees(hipStream_t s, char* scratch, const BvhBuildLayout& L, int64_t gs, const uint32_t* weight, int leaf_size,
                         int sub_start);

// bvh_finish.hip: the upward pass above the subtrees, numbering and the final arrays.  gm: work-groups of the numbering
void launch_bvh_top_upward(hipStream_t s, char* scratch, const BvhBuildLayout& L, const uint32_t* weight);
void launch_bvh_emit(hipStream_t s, char* scratch, const BvhBuildLayout& L, dim3 gm, void* geom0, void* geom1, void* link,
                     int* depth_out, uint32_t* mass_out, float2* size_out);
void launch_bvh_emit_gather(hipStream_t s, char* scratch, const BvhBuildLayout& L, dim3 gm, void* geom0, void* geom1, void* link,
                            int* depth_out, uint32_t* mass_out, float2* size_out, const GatherArgs<float>& gather);

}  // namespace nbody
