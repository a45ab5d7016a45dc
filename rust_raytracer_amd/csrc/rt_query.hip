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

// ---------------------------------------------------------------------------------------------
// Occlusion.  One lane per segment walks the OP form of the scene program with the interval (t_lo, t_hi) FIXED: OP_BOUNDS
// with the reference's Williams test and that interval, OP_GROUP as the no-op it is for every interpreter but
// k_wf_prims<GROUPS>, so a primitive is reached iff every reference ancestor box lets the segment through (DESIGN.md §14:
// the existence argument under the reference's wrong boxes, SURVEY B-8).  Spheres and quads run their own reference tests with
// the strict ends; a mesh op is searched by mesh_any_hit.  The lane leaves at the first accepted primitive.  Sky and Sun
// never occlude.
// ---------------------------------------------------------------------------------------------
// Any-hit search of one mesh instance over its 4-wide quantised nodes (MeshNode4qc), k_wf_mesh's node step without the
// ordering: the segment is fixed, so no entry distances are kept and a stack entry is the 4-B child reference (half of
// k_wf_mesh's LDS per level).  The f32 culling ray starts where the segment enters the mesh's box (the nodes' padding covers
// the slab test's rounding for such origins, rt_scene.h BvhNode4f), the back-face cone word culls for meshes that do not
// hit back faces, and the leaves run the exact object-space Moeller-Trumbore test of mesh_traverse with the strict ends.
// stack: this lane's column of the workgroup's LDS stack, entry k at stack[k * 256].
template <typename R>
RT_DEV bool mesh_any_hit(const SceneView<R>& sc, const MeshInst& mi, const Bounds<R>& rb, const Ray<R>& ray, R t_lo, R t_hi, int* stack,
                         int levels, uint32_t cones_on) {
    if (!(rb.lo[0] <= rb.hi[0])) return false;  // a mesh without triangles
    // the part of the segment inside the mesh's box, like k_wf_mesh<MULTI>
    R t_enter, t_exit;
    const CullRay<R> cr = make_cull_ray(ray, rb.lo, rb.hi, t_lo, t_enter, t_exit);
    if (span_misses(t_enter, t_exit, t_hi)) return false;
    const float tmax32 = f32_at_least(t_hi - cr.t_shift);
    const bool hit_back = (mi.flags & RT_MESH_HIT_BACK_FACES) != 0u;
    const uint32_t dirq = quantise_dir(ray.d, cones_on != 0u && !hit_back);
    const MeshNode4qc* nodesq = sc.nodes4q;
    const TriRec<R>* tris = sc.tris;  // leaf codes hold absolute triangle slots
    int32_t node = int32_t(mi.node4_base);
    int sp = 0;
    for (;;) {
        if (node >= 0) {
            // five 16-B loads from one line
            const uint4* nd = reinterpret_cast<const uint4*>(nodesq + node);
            const uint4 h0 = nd[0], h1 = nd[1], h2 = nd[2];
            const int4 cc = *reinterpret_cast<const int4*>(nd + 3);
            int32_t ch[4];
            float nr[4];
            node4q_cull_cones(dirq, nd[4], cc, ch);
            const uint32_t entered = node4q_entries(h0, h1, h2, cr, tmax32, ch, nr);
            int32_t next = kEmptyChild;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((entered >> k) & 1u) {
                    if (next != kEmptyChild && sp < levels) { stack[sp * 256] = next; sp++; }  // sp < levels always: the bound is the tree's worst case
                    next = ch[k];
                }
            }
            if (next != kEmptyChild) { node = next; continue; }
        } else {
            const uint32_t code = uint32_t(~node);
            const uint32_t first = code >> 3, count = (code & 7u) + 1u;
            for (uint32_t k = 0; k < count; k++) {
                R t = R(0), u = R(0), v = R(0);
                if (tri_test(tris[first + k], ray.o, ray.d, hit_back, t, u, v) && !(t <= t_lo || t_hi <= t)) return true;
            }
        }
        if (sp == 0) return false;
        sp--;
        node = stack[sp * 256];
    }
}

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
    Ray<R> cur = wray;
    int32_t pc = 0;
    bool occluded = false;
    for (;;) {
        const Op op = sc.ops[pc];
        if (op.type == OP_END) break;
        switch (op.type) {
            case OP_BOUNDS:
                if (!test_bounding_box(sc.bounds[op.arg], cur, t_lo, t_hi)) {
                    pc = op.skip;
                    continue;
                }
                break;
            case OP_XFORM_PUSH: {
                const Xform<R>& x = sc.xforms[op.arg];
                cur = make_ray(xform_apply(x.inv, cur.o, R(1)), xform_apply(x.inv, cur.d, R(0)));
                break;
            }
            case OP_XFORM_POP:
                cur = ray_in_chain(sc, wray, op.chain);
                break;
            case OP_SPHERE: {
                R t;
                occluded = sphere_test<R, false>(sc.spheres[op.arg], cur, t_lo, t_hi, t);
                break;
            }
            case OP_PLANE: {
                R t, u, v;
                occluded = plane_test<R, false>(sc.planes[op.arg], cur, t_lo, t_hi, t, u, v);
                break;
            }
            case OP_MESH:
                occluded = mesh_any_hit<R>(sc, sc.meshes[op.arg], sc.mesh_bounds[op.arg], cur, t_lo, t_hi, stack, levels, cones_on);
                break;
            default:  // OP_GROUP: the op form behind it is walked; OP_SKY / OP_SUN never occlude
                break;
        }
        if (occluded) break;
        pc++;
    }
    out[i] = occluded ? uint8_t(1) : uint8_t(0);
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
