// rt_bake.hip — ambient occlusion at surface points (include/rt_mi355.h: rt_bake_visibility).  A translation
// unit of its own: neither the render kernels nor the query kernels change.  One wave bakes one point: each lane draws its
// sample's direction in registers, walks the scene with segment_occluded (rt_query.h, the walk of k_rq_occluded) and the wave
// reduces; no ray is ever written to memory.
#include <hip/hip_runtime.h>

#include <limits>

#include "rt_bake.h"
#include "rt_device.h"
#include "rt_query.h"

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

}  // namespace rt
