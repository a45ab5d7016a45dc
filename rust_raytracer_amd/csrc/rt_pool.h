// rt_pool.h — the path pool and the counters of a pass over it, as the wavefront and search kernels take them
// (rt_wavefront.h) and as the scene's workspaces hold them (rt_scene_host.h).  Plain structs, no device code.
#pragma once
#include <cstdint>

namespace rt {

template <typename R>
struct WfPool {
    uint32_t capacity;
    R *ox, *oy, *oz, *dx, *dy, *dz;  // current ray, world space
    R *tr, *tg, *tb;                 // throughput: product of the weights so far (the radiance exists only at the terminal)
    uint64_t* rng;                   // stream state
    uint64_t* sample;                // sample index within the current replica group
    uint32_t* depth;                 // remaining depth (the `depth` argument of ray_color)
    R *ht, *hu, *hv;                 // closest hit: t, (u, v)
    int32_t *hpc, *htri;             // op that produced it (-1 none), triangle slot
};

struct WfCounters {
    uint32_t n_in;        // entries of the current queue
    uint32_t n_out;       // entries appended to the next queue
    uint32_t cursor;      // next queue entry to hand out (persistent intersect / mesh kernel)
    uint32_t n_mesh;      // entries of the mesh queue (paths whose ray enters a deferred mesh's box)
    unsigned long long next_sample;  // next sample (within the group) to start
    uint32_t n_mesh_next; // fused shade + prims: entries of the NEXT iteration's mesh queue (k_wf_advance moves it to n_mesh); 0 otherwise
};

}  // namespace rt
