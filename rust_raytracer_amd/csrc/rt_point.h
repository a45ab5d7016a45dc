// rt_point.h — point queries: the launcher of k_pq_closest, called by the host side of the queries (both in rt_point.hip), and the exact
// closest-point arithmetic, each routine written once: closest_on_triangle, the parallelogram as two triangles, the sphere,
// and the distance-ordered search of one mesh instance (mesh_closest).
// Definition of the result: include/rt_mi355.h (rt_closest_points), DESIGN.md §20.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rt_mi355.h"
#include "rt_device.h"
#include "rt_scene.h"

namespace rt {

// Tables of the point-query workspace (not part of SceneView: no render kernel's arguments change).
template <typename R>
struct PqTables {
    const int32_t* op_node;     // CompiledScene::op_node
    const uint32_t* tri_order;  // CompiledScene::tri_order: leaf slot -> the mesh's own triangle
    const R* chain_scale;       // per transform chain: the scale s of its (similarity) linear part, f64 rounded to R
};

// Levels of the per-lane mesh traversal stack (CompiledScene::max_bvh4_stack + 1), 8 B each: up to 32 levels run 256-lane
// workgroups, up to kPqMaxStackLevels 128-lane ones, 64 KB of LDS either way.
constexpr int kPqMaxStackLevels = 64;
// n points (n x 3 doubles) -> n RtPointHit; d_max_distance may be NULL (+inf).  d_counts != NULL: the counting variant, which
// also writes (nodes visited, triangles tested) per point.
template <typename R>
hipError_t pq_closest_launch(const SceneView<R>& sc, const PqTables<R>& tb, const double* d_points, const double* d_max_distance, uint32_t n,
                             int stack_levels, RtPointHit* d_out, uint32_t* d_counts, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Closest point of the segment a + t e, t in [0, 1], to q: the squared distance, the point in c.  A zero-length segment takes
// t = 0.
template <typename R> RT_DEV R closest_on_segment(V3<R> a, V3<R> e, V3<R> q, V3<R>& c) {
    const R ee = dot(e, e);
    R t = ee > R(0) ? dot(q - a, e) / ee : R(0);
    t = t < R(0) ? R(0) : (t > R(1) ? R(1) : t);
    c = a + e * t;
    return length_squared(q - c);
}

// Closest point of the triangle (v0, v0 + e1, v0 + e2) to q: the distance, the point in c.  With n = e1 x e2 the projection of
// q is v0 + (a e1 + b e2) with a |n|^2 = ((q - v0) x e2) . n and b |n|^2 = (e1 x (q - v0)) . n; if it lies inside all three
// edges the answer is the plane distance, otherwise the nearest of the three edge segments.  Finite, and never below the true
// distance by more than rounding, for zero-area triangles too (|n|^2 = 0 goes to the edges).
template <typename R> RT_DEV R closest_on_triangle(V3<R> v0, V3<R> e1, V3<R> e2, V3<R> q, V3<R>& c) {
    const V3<R> p = q - v0;
    const V3<R> n = cross(e1, e2);
    const R nn = dot(n, n);
    const R a = dot(cross(p, e2), n), b = dot(cross(e1, p), n);
    if (nn > R(0) && a >= R(0) && b >= R(0) && a + b <= nn) {
        const R h = dot(p, n);
        c = q - n * (h / nn);
        return fabs(h) / sqrt(nn);
    }
    V3<R> c1, c2;
    R d2 = closest_on_segment(v0, e1, q, c);
    const R d2b = closest_on_segment(v0, e2, q, c1);
    const R d2c = closest_on_segment(v0 + e1, e2 - e1, q, c2);
    if (d2b < d2) { d2 = d2b; c = c1; }
    if (d2c < d2) { d2 = d2c; c = c2; }
    return sqrt(d2);
}

// The parallelogram centre +- u +- v as its two triangles (corner, 2u, 2v) and (corner + 2u + 2v, -2u, -2v): exact for
// non-orthogonal u, v, where clamping in skewed coordinates is not.
template <typename R> RT_DEV R closest_on_plane_prim(const PlanePrim<R>& pl, V3<R> q, V3<R>& c) {
    const V3<R> corner = ld3(pl.corner), u2 = ld3(pl.u) * R(2), v2 = ld3(pl.v) * R(2);
    V3<R> c1;
    R d = closest_on_triangle(corner, u2, v2, q, c);
    const R d1 = closest_on_triangle((corner + u2) + v2, -u2, -v2, q, c1);
    if (d1 < d) { d = d1; c = c1; }
    return d;
}

// | |q - centre| - r |, r = |radius| (a hollow sphere carries a negative radius: the surface is the same); the point on the
// sphere towards q, towards +x when q is the centre; `outward` = (c - centre) / r, away from the centre for either sign.
template <typename R> RT_DEV R closest_on_sphere(const SpherePrim<R>& s, V3<R> q, V3<R>& c, V3<R>& outward) {
    const V3<R> centre = ld3(s.center), v = q - centre;
    const R len = length(v), r = fabs(s.radius);
    outward = len > R(0) ? v / len : mk<R>(1, 0, 0);
    c = centre + outward * r;
    return fabs(len - r);
}

// Object-space squared radius of the search for a best WORLD distance `best_w` under the chain scale s, rounded up, and never
// zero: at best_w = 0 (a query point on the surface) every box that contains the point (bound 0) is still entered, so every
// triangle tied at distance 0 is seen.
template <typename R> RT_DEV R pq_radius2(R best_w, R s) {
    const R r = best_w / s;
    return r * r * (R(1) + Lim<R>::eps() * R(8)) + (sizeof(R) == 8 ? R(1e-300) : R(1e-37));
}

// Distance-ordered search of one mesh instance over its 4-wide quantised nodes: a child is entered iff its lower bound
// (node4q_dist2) is below the squared search radius, the entered children are sorted nearest first, the nearest is continued
// with and the others are pushed, farthest first, as (child, f32 bound rounded down); a popped entry whose bound has been
// overtaken by then is dropped.  Leaves run closest_on_triangle; a candidate replaces the best iff its world distance s * d is
// strictly smaller, or equal to that of a triangle of this same mesh op with a higher index in the mesh's own order
// (tri_order): among tied triangles of one mesh the answer then does not depend on the shape of the tree (a tree built on the
// device, a tree kept by rt_scene_update).  stack: this lane's column of the workgroup's LDS stack, entry k at stack[k * stride].
template <typename R, bool STATS>
RT_DEV void mesh_closest(const SceneView<R>& sc, const MeshInst& mi, const Bounds<R>& mb, const uint32_t* tri_order, V3<R> q, R s, uint2* stack,
                         uint32_t stride, int levels, R& best_w, int32_t& best_tri, uint32_t& n_nodes, uint32_t& n_tris) {
    if (!(mb.lo[0] <= mb.hi[0])) return;  // a mesh without triangles
    R r2 = pq_radius2(best_w, s);
    if (!(box_dist2_below(ld3(mb.lo), ld3(mb.hi), q) < r2)) return;
    const MeshNode4qc* nodesq = sc.nodes4q;
    const TriRec<R>* tris = sc.tris;  // leaf codes hold absolute triangle slots
    int32_t node = int32_t(mi.node4_base);
    int sp = 0;
    bool mine = false;     // the best so far is a triangle of this mesh op,
    uint32_t mine_id = 0;  // this one of the mesh's own
    for (;;) {
        if (node >= 0) {
            if (STATS) n_nodes++;
            // four 16-B loads from one line
            const uint4* nd = reinterpret_cast<const uint4*>(nodesq + node);
            const uint4 h0 = nd[0], h1 = nd[1], h2 = nd[2];
            const int4 cc = *reinterpret_cast<const int4*>(nd + 3);
            int32_t ch[4] = {cc.x, cc.y, cc.z, cc.w};
            R lb[4];
            float key[4];
            node4q_dist2(h0, h1, h2, q, ch, lb);
#pragma unroll
            for (int k = 0; k < 4; k++) key[k] = lb[k] < r2 ? f32_at_most(lb[k]) : kNoEntry;
            RT_SORT4_NEAREST_FIRST(key, ch)
#pragma unroll
            for (int k = 3; k >= 1; k--) {
                if (key[k] < kNoEntry && sp < levels) {  // sp < levels always: the bound is the tree's worst case
                    stack[uint32_t(sp) * stride] = make_uint2(uint32_t(ch[k]), __float_as_uint(key[k]));
                    sp++;
                }
            }
            if (key[0] < kNoEntry) { node = ch[0]; continue; }
        } else {
            const uint32_t code = uint32_t(~node);
            const uint32_t first = code >> 3, count = (code & 7u) + 1u;
            for (uint32_t k = 0; k < count; k++) {
                const TriRec<R>& tr = tris[first + k];
                V3<R> c;
                const R dw = s * closest_on_triangle(ld3(tr.v0), ld3(tr.e1), ld3(tr.e2), q, c);
                if (STATS) n_tris++;
                if (dw <= best_w) {  // rarely true: the index is read only then
                    const uint32_t id = tri_order[first + k];
                    if (dw < best_w || (mine && id < mine_id)) {
                        best_w = dw;
                        best_tri = int32_t(first + k);
                        mine = true;
                        mine_id = id;
                        r2 = pq_radius2(best_w, s);
                    }
                }
            }
        }
        for (;;) {
            if (sp == 0) return;
            sp--;
            const uint2 e = stack[uint32_t(sp) * stride];
            if (R(__uint_as_float(e.y)) < r2) { node = int32_t(e.x); break; }
        }
    }
}

}  // namespace rt
