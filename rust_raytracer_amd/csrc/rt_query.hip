// rt_query.hip — ray queries: closest hit and occlusion for rays the caller supplies (include/rt_mi355.h: rt_trace_rays,
// rt_occluded): the kernels, their launchers, the host side (workspace, chunk loops) and the entry points.  A
// translation unit of its own: the render kernels in rt_kernels.hip are not touched.
//   closest hit:  k_rq_load writes the rays into a path pool, the scene's own search kernels run one pass over it
//                 (rt_kernels.hip, query_search_pass), k_rq_resolve turns the hit records into RtRayHit;
//   occlusion:    k_rq_occluded, an any-hit walk of the scene program that leaves at the first accepted primitive.
// rq_tables and rq_chunk serve point queries (rt_point.hip) and lightmaps (rt_lightmap.hip) too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <variant>

#include "rt_device.h"
#include "rt_query.h"
#include "rt_scene_host.h"

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

// ---------------------------------------------------------------------------------------------
// Host side: the query workspace of a scene (RtScene::Query, rt_scene_host.h), the chunk loops and the entry points
// ---------------------------------------------------------------------------------------------
uint32_t rq_chunk() { return std::min<uint32_t>(1u << 28, std::max<uint32_t>(64u, env_u32("RT_RQ_CHUNK", 1u << 22))); }

// Counters and (closest hit: `pool`) a pool of at least `capacity` slots in R.
template <typename R>
int rq_ensure(RtScene* s, uint32_t capacity, bool pool) {
    RtScene::Query& q = s->rq;
    if (int st = q.d_ctr.reserve(sizeof(WfCounters))) return st;
    if (int st = q.h_ctr.reserve(sizeof(WfCounters))) return st;
    const auto* have = std::get_if<PoolPair<R>>(&q.pools);
    if (!pool || (have && (*have)[0].view.capacity >= capacity)) return RT_OK;
    q.pools = std::monostate{};
    PoolPair<R> pp;  // the arrays a query does not use stay NULL
    if (int st = build_pool(pp[0], capacity, false, 1, "ray-query pool does not fit in device memory (RT_RQ_CHUNK sets its size)")) return st;
    q.pools = std::move(pp);
    return RT_OK;
}

// op -> node and leaf slot -> triangle tables of the scene as it stands (uploaded again after an rt_scene_update)
int rq_tables(RtScene* s, hipStream_t stream) {
    RtScene::Query& q = s->rq;
    if (q.tables_generation == s->generation && q.op_node) return RT_OK;
    q.op_node.reset();
    q.tri_order.reset();
    const CompiledScene& cs = s->compiled;
    if (int st = q.op_node.reserve(std::max<size_t>(1, cs.op_node.size()) * 4)) return st;
    if (int st = q.tri_order.reserve(std::max<size_t>(1, cs.tri_order.size()) * 4)) return st;
    if (!cs.op_node.empty()) HIP_TRY(hipMemcpyAsync(q.op_node, cs.op_node.data(), cs.op_node.size() * 4, hipMemcpyHostToDevice, stream));
    if (!cs.tri_order.empty()) HIP_TRY(hipMemcpyAsync(q.tri_order, cs.tri_order.data(), cs.tri_order.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    q.tables_generation = s->generation;
    return RT_OK;
}

// n rays in chunks: (host variant: through the staging buffer) k_rq_load -> search pass -> k_rq_resolve.
template <typename R>
int trace_rays_typed(RtScene* s, DeviceScene<R>& ds, uint64_t n, const double* origins, const double* dirs, RtRayHit* out, bool host,
                     hipStream_t stream) {
    RtScene::Query& q = s->rq;
    const uint32_t chunk = rq_chunk();
    if (int st = rq_ensure<R>(s, uint32_t(std::min<uint64_t>(n, chunk)), true)) return st;
    if (int st = rq_tables(s, stream)) return st;
    const PathPool<R>& pl = std::get<PoolPair<R>>(q.pools)[0];
    const WfPool<R>& full = pl.view;
    const RqPool<R> rp{full.ox, full.oy, full.oz, full.dx, full.dy, full.dz, full.ht, full.hu, full.hv, full.hpc, full.htri};
    const RqTables tb{q.op_node, q.tri_order};
    ChunkTimes t;
    auto launch = [&](uint64_t, uint32_t m, const void* const* d_in, void* d_out) -> int {
        HIP_TRY(rq_load_launch<R>(rp, static_cast<const double*>(d_in[0]), static_cast<const double*>(d_in[1]), m, pl.queue[0], stream));
        if (int st = query_search_pass(s, ds, pl, m, stream)) return st;
        HIP_TRY(rq_resolve_launch<R>(ds.view, rp, tb, m, static_cast<RtRayHit*>(d_out), stream));
        return RT_OK;
    };
    if (int st = run_chunks(q.stage, n, chunk, host, {{origins, 24}, {dirs, 24}}, out, sizeof(RtRayHit), stream, launch, &t)) return st;
    record_query_stats<R>(q.stats, t, n);
    return RT_OK;
}

template <typename R>
int occluded_typed(RtScene* s, DeviceScene<R>& ds, uint64_t n, const double* origins, const double* dirs, const double* t_min,
                   const double* t_max, uint8_t* out, bool host, hipStream_t stream) {
    RtScene::Query& q = s->rq;
    const int levels = s->compiled.meshes.empty() ? 1 : int(s->compiled.max_bvh4_stack) + 1;
    if (levels > kRqMaxStackLevels) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the occlusion kernel's LDS traversal stack");
    const uint32_t cones_on = env_u32("RT_WF_CONES", 1) != 0 ? 1u : 0u;
    const uint32_t chunk = rq_chunk();
    if (int st = rq_ensure<R>(s, uint32_t(std::min<uint64_t>(n, chunk)), false)) return st;
    ChunkTimes t;
    auto launch = [&](uint64_t, uint32_t m, const void* const* d_in, void* d_out) -> int {
        HIP_TRY(rq_occluded_launch<R>(ds.view, static_cast<const double*>(d_in[0]), static_cast<const double*>(d_in[1]), static_cast<const double*>(d_in[2]),
                                      static_cast<const double*>(d_in[3]), m, levels, cones_on, static_cast<uint8_t*>(d_out), stream));
        return RT_OK;
    };
    if (int st = run_chunks(q.stage, n, chunk, host, {{origins, 24}, {dirs, 24}, {t_min, 8}, {t_max, 8}}, out, 1, stream, launch, &t)) return st;
    record_query_stats<R>(q.stats, t, n);
    return RT_OK;
}

}  // namespace rt

extern "C" {

static int trace_rays_impl(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, uint32_t precision, RtRayHit* out,
                           bool host, void* stream, const char* who) {
    using namespace rt;
    return ray_query_run(scene, precision, who, [&](RtScene* s, auto& ds) -> int {
        if (n == 0) return RT_OK;
        if (!origins || !dirs || !out) return set_err(RT_E_INVALID, std::string(who) + ": NULL array");
        return trace_rays_typed(s, ds, n, origins, dirs, out, host, stream ? static_cast<hipStream_t>(stream) : s->stream);
    });
}

static int occluded_impl(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, const double* t_min, const double* t_max,
                         uint32_t precision, uint8_t* out, bool host, void* stream, const char* who) {
    using namespace rt;
    return ray_query_run(scene, precision, who, [&](RtScene* s, auto& ds) -> int {
        if (n == 0) return RT_OK;
        if (!origins || !dirs || !out) return set_err(RT_E_INVALID, std::string(who) + ": NULL array");
        return occluded_typed(s, ds, n, origins, dirs, t_min, t_max, out, host, stream ? static_cast<hipStream_t>(stream) : s->stream);
    });
}

int rt_trace_rays(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, uint32_t precision, RtRayHit* hits_out) {
    return trace_rays_impl(scene, n, origins, dirs, precision, hits_out, true, nullptr, "rt_trace_rays");
}
int rt_trace_rays_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs, uint32_t precision,
                         RtRayHit* d_hits_out, void* stream) {
    return trace_rays_impl(scene, n, d_origins, d_dirs, precision, d_hits_out, false, stream, "rt_trace_rays_device");
}
int rt_occluded(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, const double* t_min, const double* t_max,
                uint32_t precision, uint8_t* out) {
    return occluded_impl(scene, n, origins, dirs, t_min, t_max, precision, out, true, nullptr, "rt_occluded");
}
int rt_occluded_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs, const double* d_t_min,
                       const double* d_t_max, uint32_t precision, uint8_t* d_out, void* stream) {
    return occluded_impl(scene, n, d_origins, d_dirs, d_t_min, d_t_max, precision, d_out, false, stream, "rt_occluded_device");
}
int rt_ray_query_stats(const RtScene* scene, RtRayQueryStats* out) {
    if (!scene || !out) return rt::set_err(RT_E_INVALID, "rt_ray_query_stats: NULL argument");
    *out = scene->rq.stats;
    return RT_OK;
}

}  // extern "C"
