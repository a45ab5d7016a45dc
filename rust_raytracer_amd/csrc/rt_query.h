// rt_query.h — launchers of the ray-query kernels, called by the host side of the queries (both in rt_query.hip), and the
// occlusion walk of the scene program (segment_occluded), one definition for every kernel that asks "is this segment blocked".
// Definitions of the results: include/rt_mi355.h (rt_trace_rays, rt_occluded), DESIGN.md §14.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rt_mi355.h"
#include "rt_device.h"
#include "rt_scene.h"

namespace rt {

// The arrays of a WfPool<R> (rt_pool.h) that a query touches: the ray the search kernels read and the hit record they leave.
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

// ---------------------------------------------------------------------------------------------
// Occlusion walk, the one definition shared by k_rq_occluded (rt_query.hip) and k_bake_visibility (rt_bake.hip).  One lane
// per segment walks the OP form of the scene program with the interval (t_lo, t_hi) FIXED: OP_BOUNDS
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

// true iff the segment wray.o + t * wray.d, t in (t_lo, t_hi), is blocked.  stack / levels / cones_on: see mesh_any_hit.
template <typename R>
RT_DEV bool segment_occluded(const SceneView<R>& sc, const Ray<R>& wray, R t_lo, R t_hi, int* stack, int levels, uint32_t cones_on) {
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
    return occluded;
}

}  // namespace rt
