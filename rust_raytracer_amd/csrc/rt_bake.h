// rt_bake.h — launcher of the ambient-occlusion bake, called by the host side of the bake (both in rt_bake.hip), and the
// parameter rules that rt_bake_lightmap (rt_lightmap.hip) checks too.
// Definition of the result: include/rt_mi355.h (rt_bake_visibility), DESIGN.md §15.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/rt_mi355.h"
#include "rt_scene.h"

namespace rt {

// The points of one chunk.  Position and normal of point p (p = 0 .. n-1 within the chunk) are three doubles each at
// pos + p * pos_stride and nrm + p * nrm_stride (bytes): two packed n x 3 arrays (stride 24) and an array of RtRayHit
// (pos at offset 8, normal at offset 32, stride 96) are the same kernel.  flags: NULL, or the RT_RAY_* word of point p at
// flags + p * flags_stride; a record without RT_RAY_HIT or with RT_RAY_ENVIRONMENT is skipped (visibility 1, bent 0).
struct BakePoints {
    const unsigned char* pos;
    const unsigned char* nrm;
    const unsigned char* flags;
    uint32_t pos_stride, nrm_stride, flags_stride;
    uint32_t n;
    uint64_t first;  // index of point 0 within the whole call: the generator is keyed by first + p, not by p
};

// out[p] for the n points of `pts`: `samples` cosine-weighted directions about the normal, each tested over (bias, max_distance)
// by segment_occluded (rt_query.h).  stack_levels as for rq_occluded_launch (at most kRqMaxStackLevels).
template <typename R>
hipError_t bake_visibility_launch(const SceneView<R>& sc, const BakePoints& pts, uint32_t samples, uint64_t seed, double bias,
                                  double max_distance, int stack_levels, uint32_t cones_on, RtBakeResult* d_out, hipStream_t stream);

// The rules of samples, bias and max_distance; prefix: what the message starts with, "<entry point>: ".
int bake_params_check(const RtBakeParams& bp, const std::string& prefix);

}  // namespace rt
