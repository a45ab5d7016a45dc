// rt_query.h — launchers of the ray-query kernels (rt_query.hip), called by the C ABI in rt_kernels.hip.
// Definitions of the results: include/rt_mi355.h (rt_trace_rays, rt_occluded), DESIGN.md §14.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rt_mi355.h"
#include "rt_scene.h"

namespace rt {

// The arrays of a WfPool<R> (rt_wavefront.h) that a query touches: the ray the search kernels read and the hit record
// they leave.  A view of its own, so that this translation unit does not need the scheduler's header.
template <typename R>
struct RqPool {
    R *ox, *oy, *oz, *dx, *dy, *dz;
    R *ht, *hu, *hv;
    int32_t *hpc, *htri;
};

// Tables of the query workspace (not part of SceneView: no render kernel's arguments change).
struct RqTables {
    const int32_t* op_node;     // CompiledScene::op_node
    const uint32_t* tri_order;  // CompiledScene::tri_order: leaf slot -> the mesh's own triangle
};

// Rays i = 0 .. n-1 (n x 3 doubles each) -> pool slots i, queue[i] = i.
template <typename R>
hipError_t rq_load_launch(const RqPool<R>& pool, const double* d_origins, const double* d_dirs, uint32_t n, uint32_t* queue,
                          hipStream_t stream);
// Hit records of slots 0 .. n-1 -> out[0 .. n).
template <typename R>
hipError_t rq_resolve_launch(const SceneView<R>& sc, const RqPool<R>& pool, const RqTables& tb, uint32_t n, RtRayHit* d_out,
                             hipStream_t stream);
// Any-hit query of n segments; d_tmin / d_tmax may be NULL (0.001 / +inf).  stack_levels: entries of the per-lane mesh
// traversal stack (CompiledScene::max_bvh4_stack + 1; at most kRqMaxStackLevels).
constexpr int kRqMaxStackLevels = 64;  // 64 KB of LDS per workgroup
template <typename R>
hipError_t rq_occluded_launch(const SceneView<R>& sc, const double* d_origins, const double* d_dirs, const double* d_tmin,
                              const double* d_tmax, uint32_t n, int stack_levels, uint32_t cones_on, uint8_t* d_out,
                              hipStream_t stream);

}  // namespace rt
