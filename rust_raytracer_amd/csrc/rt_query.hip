// rt_query.hip — ray queries: closest hit and occlusion for rays the caller supplies (include/rt_mi355.h: rt_trace_rays,
// rt_occluded).  A translation unit of its own: the render kernels in rt_kernels.hip are not touched.
//   closest hit:  k_rq_load writes the rays into a path pool, the scene's own search kernels run one pass over it
//                 (rt_kernels.hip, query_search_pass), k_rq_resolve turns the hit records into RtRayHit;
//   occlusion:    k_rq_occluded, an any-hit walk of the scene program that leaves at the first accepted primitive.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "rt_device.h"
#include "rt_query.h"

namespace rt {

template <typename R>
__global__ void __launch_bounds__(256) k_rq_load(RqPool<R> pool, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                 uint32_t n, uint32_t* __restrict__ queue) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* o = origins + 3 * size_t(i);
    const double* d = dirs + 3 * size_t(i);
    pool.ox[i] = R(o[0]); pool.oy[i] = R(o[1]); pool.oz[i] = R(o[2]);
    pool.dx[i] = R(d[0]); pool.dy[i] = R(d[1]); pool.dz[i] = R(d[2]);
    queue[i] = i;
}

// The geometric half of resolve_hit (rt_device.h), same arithmetic in the same order: HitRecord::hit_pos / ::normal / ::u /
// ::v / ::front_face as the reference leaves them after Transform::test.  No texture is evaluated and no normal map applied;
// sphere and sky (u, v) are always computed (the render computes them only for materials that read them).
template <typename R>
__global__ void __launch_bounds__(256) k_rq_resolve(SceneView<R> sc, RqPool<R> pool, RqTables tb, uint32_t n, RtRayHit* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RtRayHit h;
    h.t = double(Lim<double>::inf());
    for (int k = 0; k < 3; k++) { h.pos[k] = 0.0; h.normal[k] = 0.0; }
    h.u = 0.0; h.v = 0.0;
    h.material = -1; h.node = -1; h.prim = -1;
    h.flags = 0u;
    h._reserved = 0ull;
    const int32_t pc = pool.hpc[i];
    if (pc >= 0) {
        const Op op = sc.ops[pc];
        const R t = pool.ht[i], bu = pool.hu[i], bv = pool.hv[i];
        const Ray<R> wray = make_ray(mk<R>(pool.ox[i], pool.oy[i], pool.oz[i]), mk<R>(pool.dx[i], pool.dy[i], pool.dz[i]));
        const Ray<R> ray = ray_in_chain(sc, wray, op.chain);
        V3<R> pos, outward;
        R u = R(0), v = R(0);
        int32_t material;
        double t_out = double(t);
        uint32_t flags = RT_RAY_HIT;
        switch (op.type) {
            case OP_SPHERE: {  // sphere.rs:64-93
                const SpherePrim<R>& s = sc.spheres[op.arg];
                pos = ray_at(ray, t);
                outward = (pos - ld3(s.center)) / s.radius;
                material = s.material;
                R theta = uv_acos(outward.y);
                R phi = uv_atan2(-outward.z, outward.x) + pi<R>();
                u = phi / (R(2) * pi<R>());
                v = theta / pi<R>();
                break;
            }
            case OP_PLANE: {  // plane.rs:81-100
                const PlanePrim<R>& p = sc.planes[op.arg];
                pos = ray_at(ray, t);
                outward = ld3(p.normal);
                material = p.material;
                u = bu;
                v = bv;
                break;
            }
            case OP_MESH: {  // mesh.rs:103-162
                const MeshInst& mi = sc.meshes[op.arg];
                const int32_t tri = pool.htri[i];
                const TriAttr<R>& at = sc.attrs[tri];
                pos = ray_at(ray, t);
                R w = R(1) - bu - bv;
                if (mi.flags & RT_MESH_FLAT_SHADING) {
                    const TriRec<R>& tr = sc.tris[tri];
                    outward = to_unit(cross(ld3(tr.e1), ld3(tr.e2)));
                } else {
                    outward = ld3(at.n0) * w + ld3(at.n1) * bu + ld3(at.n2) * bv;  // not normalised (SURVEY B-4)
                }
                if (at.has_uv) {
                    u = at.uv0[0] * w + at.uv1[0] * bu + at.uv2[0] * bv;
                    v = at.uv0[1] * w + at.uv1[1] * bu + at.uv2[1] * bv;
                }
                material = mi.material;
                h.prim = int32_t(tb.tri_order[tri]);
                break;
            }
            case OP_SKY: {  // sky.rs:35-51
                pos = ray_at(ray, Lim<R>::inf());
                V3<R> unit_dir = to_unit(ray.d);
                outward = -unit_dir;
                material = op.arg;
                u = uv_atan2(unit_dir.x, unit_dir.z) / (R(2) * pi<R>()) + R(0.5);
                v = dot(unit_dir, mk<R>(0, 1, 0)) / R(2) + R(0.5);
                t_out = double(Lim<double>::inf());
                flags |= RT_RAY_ENVIRONMENT;
                break;
            }
            default: {  // OP_SUN, sun.rs:45-60 (volumes are refused before any kernel runs)
                const SunPrim<R>& s = sc.suns[op.arg];
                pos = ray_at(ray, Lim<R>::max());
                outward = -to_unit(ray.d);
                material = s.material;
                t_out = DBL_MAX;
                flags |= RT_RAY_ENVIRONMENT;
                break;
            }
        }
        const bool front_face = dot(ray.d, outward) < R(0);  // object.rs:55, decided in object space
        V3<R> normal = front_face ? outward : -outward;
        // Transform::test on the way back up (transform.rs:132-133), innermost first
        const int32_t b = sc.chain_offsets[op.chain], e = sc.chain_offsets[op.chain + 1];
        for (int32_t k = e - 1; k >= b; k--) {
            const Xform<R>& x = sc.xforms[sc.chain_items[k]];
            pos = xform_apply(x.m, pos, R(1));
            normal = to_unit(xform_apply(x.m, normal, R(0)));
        }
        if (front_face) flags |= RT_RAY_FRONT_FACE;
        h.t = t_out;
        h.pos[0] = double(pos.x); h.pos[1] = double(pos.y); h.pos[2] = double(pos.z);
        h.normal[0] = double(normal.x); h.normal[1] = double(normal.y); h.normal[2] = double(normal.z);
        h.u = double(u);
        h.v = double(v);
        h.material = material;
        h.node = tb.op_node[pc];
        h.flags = flags;
    }
    out[i] = h;
}

// Occlusion: one lane per segment runs the walk of rt_query.h (segment_occluded).
template <typename R>
__global__ void __launch_bounds__(256) k_rq_occluded(SceneView<R> sc, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                     const double* __restrict__ tmin, const double* __restrict__ tmax, uint32_t n, int levels,
                                                     uint32_t cones_on, uint8_t* __restrict__ out) {
    extern __shared__ int rq_stack[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int* stack = rq_stack + threadIdx.x;
    const double* po = origins + 3 * size_t(i);
    const double* pd = dirs + 3 * size_t(i);
    const Ray<R> wray = make_ray(mk<R>(R(po[0]), R(po[1]), R(po[2])), mk<R>(R(pd[0]), R(pd[1]), R(pd[2])));
    const R t_lo = tmin ? R(tmin[i]) : R(0.001);
    const R t_hi = tmax ? R(tmax[i]) : Lim<R>::inf();
    out[i] = segment_occluded<R>(sc, wray, t_lo, t_hi, stack, levels, cones_on) ? uint8_t(1) : uint8_t(0);
}

// ---------------------------------------------------------------------------------------------
template <typename R>
hipError_t rq_load_launch(const RqPool<R>& pool, const double* d_origins, const double* d_dirs, uint32_t n, uint32_t* queue,
                          hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((k_rq_load<R>), dim3((n + 255u) / 256u), dim3(256), 0, stream, pool, d_origins, d_dirs, n, queue);
    return hipGetLastError();
}

template <typename R>
hipError_t rq_resolve_launch(const SceneView<R>& sc, const RqPool<R>& pool, const RqTables& tb, uint32_t n, RtRayHit* d_out,
                             hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((k_rq_resolve<R>), dim3((n + 255u) / 256u), dim3(256), 0, stream, sc, pool, tb, n, d_out);
    return hipGetLastError();
}

template <typename R>
hipError_t rq_occluded_launch(const SceneView<R>& sc, const double* d_origins, const double* d_dirs, const double* d_tmin,
                              const double* d_tmax, uint32_t n, int stack_levels, uint32_t cones_on, uint8_t* d_out,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (stack_levels < 1 || stack_levels > kRqMaxStackLevels) return hipErrorInvalidValue;
    const size_t lds = size_t(stack_levels) * 256 * sizeof(int);
    hipLaunchKernelGGL((k_rq_occluded<R>), dim3((n + 255u) / 256u), dim3(256), lds, stream, sc, d_origins, d_dirs, d_tmin, d_tmax, n,
                       stack_levels, cones_on, d_out);
    return hipGetLastError();
}

#define RT_RQ_INSTANTIATE(R)                                                                                                      \
    template hipError_t rq_load_launch<R>(const RqPool<R>&, const double*, const double*, uint32_t, uint32_t*, hipStream_t);        \
    template hipError_t rq_resolve_launch<R>(const SceneView<R>&, const RqPool<R>&, const RqTables&, uint32_t, RtRayHit*, hipStream_t); \
    template hipError_t rq_occluded_launch<R>(const SceneView<R>&, const double*, const double*, const double*, const double*,     \
                                              uint32_t, int, uint32_t, uint8_t*, hipStream_t);
RT_RQ_INSTANTIATE(double)
RT_RQ_INSTANTIATE(float)
#undef RT_RQ_INSTANTIATE

}  // namespace rt
