// rt_bake.hip — ambient occlusion at surface points (include/rt_mi355.h: rt_bake_visibility).  A translation
// unit of its own: neither the render kernels nor the query kernels change.  One wave bakes one point: each lane draws its
// sample's direction in registers, walks the scene with segment_occluded (rt_query.h, the walk of k_rq_occluded) and the wave
// reduces; no ray is ever written to memory.  The kernel, its launcher, the host side (chunk loop) and the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "rt_bake.h"
#include "rt_device.h"
#include "rt_query.h"
#include "rt_scene_host.h"

namespace rt {

// Sum over the 64 lanes of a wave, a butterfly with xor 32, 16, 8, 4, 2, 1 in that order: after the step with mask m every lane
// holds x[lane] + x[lane ^ m] (IEEE addition commutes, so both partners hold the same bits), and after the last step every
// lane holds ((((x + x^32) + ^16) + ^8) + ^4) + ^2) + ^1 of its own column: one fixed tree, the same in every lane.
template <typename R> RT_DEV R wave_sum(R x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}

// Workgroup = 4 waves = 4 points; sample s of a point runs in lane s % 64 of pass s / 64.
//   Rng g; g.key(seed, 0, first + p, s);  w = to_unit(normal);  onb_from_vec(w, u, v);
//   d = basis_apply(u, v, w, random_cosine(g));  visible = !segment_occluded(ray(pos, d), bias, max_distance)
// Reduction (fixed): count = popcount of the wave's ballot of `visible`, summed over passes (integers); sum = per pass the
// butterfly wave_sum over the lanes of (visible ? d : 0), in R, the passes added in ascending order.  Lane 0 writes
// visibility = double(count) / double(S), bent[k] = double(sum[k]) / double(S).
// LDS: the traversal stack of mesh_any_hit, [level][lane] (consecutive lanes in consecutive banks), levels x 256 ints.
template <typename R>
__global__ void __launch_bounds__(256) k_bake_visibility(SceneView<R> sc, BakePoints pts, uint32_t samples, uint64_t seed, R bias,
                                                         R max_distance, int levels, uint32_t cones_on, RtBakeResult* __restrict__ out) {
    extern __shared__ int bake_stack[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= pts.n) return;  // the whole wave leaves: no barrier follows
    int* stack = bake_stack + threadIdx.x;
    if (pts.flags) {
        const uint32_t f = *reinterpret_cast<const uint32_t*>(pts.flags + size_t(p) * pts.flags_stride);
        if (!(f & RT_RAY_HIT) || (f & RT_RAY_ENVIRONMENT)) {  // wave-uniform
            if (lane == 0) {
                RtBakeResult r;
                r.visibility = 1.0;
                r.bent[0] = 0.0; r.bent[1] = 0.0; r.bent[2] = 0.0;
                out[p] = r;
            }
            return;
        }
    }
    const double* pp = reinterpret_cast<const double*>(pts.pos + size_t(p) * pts.pos_stride);
    const double* pn = reinterpret_cast<const double*>(pts.nrm + size_t(p) * pts.nrm_stride);
    const V3<R> origin = mk<R>(R(pp[0]), R(pp[1]), R(pp[2]));
    const V3<R> w = to_unit(mk<R>(R(pn[0]), R(pn[1]), R(pn[2])));
    V3<R> u, v;
    onb_from_vec(w, u, v);
    const uint64_t point = pts.first + p;
    uint32_t count = 0;
    V3<R> sum = mk<R>(0, 0, 0);
    for (uint32_t s0 = 0; s0 < samples; s0 += 64u) {
        const uint32_t s = s0 + lane;
        bool visible = false;
        V3<R> d = mk<R>(0, 0, 0);
        if (s < samples) {
            Rng g;
            g.key(seed, 0u, point, s);
            d = basis_apply(u, v, w, random_cosine<R>(g));
            visible = !segment_occluded<R>(sc, make_ray(origin, d), bias, max_distance, stack, levels, cones_on);
        }
        count += uint32_t(__popcll(__ballot(visible)));
        if (!visible) d = mk<R>(0, 0, 0);
        const V3<R> pass = mk<R>(wave_sum(d.x), wave_sum(d.y), wave_sum(d.z));
        sum = sum + pass;
    }
    if (lane == 0) {
        const double S = double(samples);
        RtBakeResult r;
        r.visibility = double(count) / S;
        r.bent[0] = double(sum.x) / S; r.bent[1] = double(sum.y) / S; r.bent[2] = double(sum.z) / S;
        out[p] = r;
    }
}

template <typename R>
hipError_t bake_visibility_launch(const SceneView<R>& sc, const BakePoints& pts, uint32_t samples, uint64_t seed, double bias,
                                  double max_distance, int stack_levels, uint32_t cones_on, RtBakeResult* d_out, hipStream_t stream) {
    if (pts.n == 0) return hipSuccess;
    if (stack_levels < 1 || stack_levels > kRqMaxStackLevels || samples == 0) return hipErrorInvalidValue;
    const size_t lds = size_t(stack_levels) * 256 * sizeof(int);
    // a distance beyond R's range is "unlimited" (a conversion out of range is not defined)
    const R t_hi = max_distance > double(std::numeric_limits<R>::max()) ? std::numeric_limits<R>::infinity() : R(max_distance);
    hipLaunchKernelGGL((k_bake_visibility<R>), dim3((pts.n + 3u) / 4u), dim3(256), lds, stream, sc, pts, samples, seed, R(bias), t_hi,
                       stack_levels, cones_on, d_out);
    return hipGetLastError();
}

template hipError_t bake_visibility_launch<double>(const SceneView<double>&, const BakePoints&, uint32_t, uint64_t, double, double, int,
                                                   uint32_t, RtBakeResult*, hipStream_t);
template hipError_t bake_visibility_launch<float>(const SceneView<float>&, const BakePoints&, uint32_t, uint64_t, double, double, int,
                                                  uint32_t, RtBakeResult*, hipStream_t);

// ---------------------------------------------------------------------------------------------
// Host side: the bake workspace of a scene (RtScene::Bake, rt_scene_host.h), the chunk loop and the entry points
// ---------------------------------------------------------------------------------------------
// points per launch; the default is a guess, not a measurement
static uint32_t bake_chunk() { return std::min<uint32_t>(1u << 26, std::max<uint32_t>(1u, env_u32("RT_BAKE_CHUNK", 1u << 20))); }

int bake_params_check(const RtBakeParams& bp, const std::string& prefix) {
    if (bp.samples < 1 || bp.samples > 4096) return set_err(RT_E_INVALID, prefix + "samples must be in 1 .. 4096");
    if (!(bp.bias >= 0.0)) return set_err(RT_E_INVALID, prefix + "bias must be >= 0");
    if (!(bp.max_distance > bp.bias)) return set_err(RT_E_INVALID, prefix + "max_distance must be greater than bias");
    return RT_OK;
}

// n points in chunks.  hits: the points are RtRayHit records on the device (positions = the records, normals unused);
// host: positions / normals / out are host arrays, staged chunk by chunk.
template <typename R>
int bake_typed(RtScene* s, DeviceScene<R>& ds, uint64_t n, const double* positions, const double* normals, const RtRayHit* hits,
               const RtBakeParams& bp, RtBakeResult* out, bool host, hipStream_t stream) {
    RtScene::Bake& b = s->bake;
    const int levels = s->compiled.meshes.empty() ? 1 : int(s->compiled.max_bvh4_stack) + 1;
    if (levels > kRqMaxStackLevels) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the bake kernel's LDS traversal stack");
    const uint32_t cones_on = env_u32("RT_WF_CONES", 1) != 0 ? 1u : 0u;
    ChunkTimes t;
    auto launch = [&](uint64_t off, uint32_t m, const void* const* d_in, void* d_out) -> int {
        BakePoints pts{};
        pts.n = m;
        pts.first = off;
        if (hits) {
            const HitPoints h = hit_points(hits + off);
            pts.pos = h.pos;
            pts.nrm = h.nrm;
            pts.flags = h.flags;
            pts.pos_stride = pts.nrm_stride = pts.flags_stride = h.stride;
        } else {
            pts.pos = static_cast<const unsigned char*>(d_in[0]);
            pts.nrm = static_cast<const unsigned char*>(d_in[1]);
            pts.pos_stride = pts.nrm_stride = 24u;
        }
        HIP_TRY(bake_visibility_launch<R>(ds.view, pts, bp.samples, bp.seed, bp.bias, bp.max_distance, levels, cones_on, static_cast<RtBakeResult*>(d_out), stream));
        return RT_OK;
    };
    const std::vector<ChunkArray> in = hits ? std::vector<ChunkArray>{} : std::vector<ChunkArray>{{positions, 24}, {normals, 24}};
    if (int st = run_chunks(b.stage, n, bake_chunk(), host, in, out, sizeof(RtBakeResult), stream, launch, &t)) return st;
    record_query_stats<R>(b.stats, t, n * bp.samples);
    return RT_OK;
}

}  // namespace rt

extern "C" {

static int bake_impl(const RtScene* scene, uint64_t n, const double* positions, const double* normals, const RtRayHit* hits,
                     const RtBakeParams* params, RtBakeResult* out, bool host, void* stream, const char* who) {
    using namespace rt;
    RtBakeParams bp{};
    if (params) {
        bp = *params;
    } else {
        bp.samples = 64;
        bp.precision = RT_PRECISION_F64;
        bp.bias = 0.001;
        bp.max_distance = HUGE_VAL;
    }
    return ray_query_run(scene, bp.precision, who, [&](RtScene* s, auto& ds) -> int {
        if (int st = bake_params_check(bp, std::string(who) + ": ")) return st;
        if (n == 0) return RT_OK;
        if (!out || (hits ? false : (!positions || !normals))) return set_err(RT_E_INVALID, std::string(who) + ": NULL array");
        return bake_typed(s, ds, n, positions, normals, hits, bp, out, host, stream ? static_cast<hipStream_t>(stream) : s->stream);
    });
}

int rt_bake_visibility(const RtScene* scene, uint64_t n, const double* positions, const double* normals, const RtBakeParams* params,
                       RtBakeResult* out) {
    return bake_impl(scene, n, positions, normals, nullptr, params, out, true, nullptr, "rt_bake_visibility");
}
int rt_bake_visibility_device(const RtScene* scene, uint64_t n, const double* d_positions, const double* d_normals,
                              const RtBakeParams* params, RtBakeResult* d_out, void* stream) {
    return bake_impl(scene, n, d_positions, d_normals, nullptr, params, d_out, false, stream, "rt_bake_visibility_device");
}
int rt_bake_visibility_hits_device(const RtScene* scene, uint64_t n, const RtRayHit* d_hits, const RtBakeParams* params,
                                   RtBakeResult* d_out, void* stream) {
    using namespace rt;
    if (n != 0 && !d_hits) return set_err(RT_E_INVALID, "rt_bake_visibility_hits_device: NULL array");
    return bake_impl(scene, n, nullptr, nullptr, d_hits, params, d_out, false, stream, "rt_bake_visibility_hits_device");
}
int rt_bake_stats(const RtScene* scene, RtRayQueryStats* out) {
    if (!scene || !out) return rt::set_err(RT_E_INVALID, "rt_bake_stats: NULL argument");
    *out = scene->bake.stats;
    return RT_OK;
}

}  // extern "C"
