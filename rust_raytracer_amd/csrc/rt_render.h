// rt_render.h — what a client of the renderer may use (rt_accum.hip is the one client): the two replica renders, the
// helpers it shares with the entry points of rt_kernels.hip, and the six fields of a scene it touches.  The boundary is
// functions and not the struct (rt_scene_host.h, for the translation units that own a workspace of the scene) by choice: a
// client renders and reads six fields, and the accessors say so; with RtScene in view nothing would.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rt_mi355.h"

namespace rt {

// One segment of an adaptive accumulator's render (rt_accum_render): the resolve step goes through
// k_wf_resolve_moments; sparse: the replica groups cover the n_active pixels of `active` instead of the frame.  The caller
// dispatches on `sparse`: AdaptiveMode<false> / <true> are the two modes.
struct AdaptivePass {
    const uint32_t* active = nullptr;
    uint32_t n_active = 0;
    bool sparse = false;
    double *s1 = nullptr, *s2 = nullptr;
    uint32_t* cnt = nullptr;
};

// Renders the replicas [t_first, t_first + n) of the frame into d_rgba_out (running sum of [0, t_first) on entry):
// rt_render_device is [0, T), rt_accum_render the next n of an accumulator.
int render_replicas(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t t_first, uint32_t n,
                    double* d_rgba_out, void* stream, const AdaptivePass* ad = nullptr);
// The first-hit AOVs of the replicas [0, n_replicas) into d_out (rt_render_aov_device).
int render_aov_replicas(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                        double* d_out, void* stream);

int validate_render_args(const RtCameraDesc* camera, const RtRenderParams* params);
// total += part (first: total = part), the sums of a call that renders in several pieces
void stats_add(RtRenderStats& total, const RtRenderStats& part, bool first);

// The scene's fields a client reads ...
int scene_device(const RtScene* s);
hipStream_t scene_stream(const RtScene* s);
uint64_t scene_generation(const RtScene* s);
uint64_t scene_content_digest(const RtScene* s);
// ... and the two it also replaces: the stats of the last render, and the tail flag (rt_scene_set_tail_flag)
const RtRenderStats& scene_stats(const RtScene* s);
void scene_set_stats(RtScene* s, const RtRenderStats& stats);
int32_t* scene_tail_flag(const RtScene* s);
void scene_set_tail_flag(RtScene* s, int32_t* flag);
// Whoever waits for a render's tail is released at the latest at the end of the call: stores 1 to the flag, if there is one.
void scene_release_tail(const RtScene* s);

}  // namespace rt
