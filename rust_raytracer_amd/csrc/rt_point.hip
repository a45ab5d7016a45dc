// rt_point.hip — point queries: the closest surface point of the scene to points the caller supplies (include/rt_mi355.h:
// rt_closest_points).  A translation unit of its own: no other kernel is touched.
//   k_pq_closest: one lane per point walks the op form of the scene program without ever skipping (the reference's boxes are
//   not all correct, SURVEY B-8, so they cannot cull by distance); spheres and parallelograms run their exact tests, a mesh
//   op is searched nearest child first by mesh_closest (rt_point.h) with a radius that shrinks as candidates are found.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "rt_device.h"
#include "rt_point.h"

namespace rt {

template <typename R, bool STATS>
__global__ void __launch_bounds__(256) k_pq_closest(SceneView<R> sc, PqTables<R> tb, const double* __restrict__ points,
                                                    const double* __restrict__ max_distance, uint32_t n, int levels,
                                                    RtPointHit* __restrict__ out, uint32_t* __restrict__ counts) {
    extern __shared__ uint2 pq_stack[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint2* stack = pq_stack + threadIdx.x;
    const uint32_t stride = blockDim.x;
    const double* pq = points + 3 * size_t(i);
    const V3<R> wq = mk<R>(R(pq[0]), R(pq[1]), R(pq[2]));
    R best_w = max_distance ? R(max_distance[i]) : Lim<R>::inf();  // world distance of the best candidate so far
    int32_t best_pc = -1, best_tri = -1;
    uint32_t n_nodes = 0u, n_tris = 0u;
    V3<R> cur = wq;
    // every lane walks every op, so the program counter is wave-uniform: the op comes through scalar loads
    for (int32_t pc = 0;; pc++) {
        const int32_t upc = __builtin_amdgcn_readfirstlane(pc);
        const auto* ops = as_const_mem(sc.ops);
        const int32_t type = ops[upc].type, arg = ops[upc].arg, chain = ops[upc].chain;
        if (type == OP_END) break;
        switch (type) {
            case OP_XFORM_PUSH:
                cur = xform_apply(sc.xforms[arg].inv, cur, R(1));
                break;
            case OP_XFORM_POP:
                cur = point_in_chain(sc, wq, chain);
                break;
            case OP_SPHERE: {
                V3<R> c, outward;
                const R dw = tb.chain_scale[chain] * closest_on_sphere(sc.spheres[arg], cur, c, outward);
                if (dw < best_w) { best_w = dw; best_pc = upc; }
                break;
            }
            case OP_PLANE: {
                V3<R> c;
                const R dw = tb.chain_scale[chain] * closest_on_plane_prim(sc.planes[arg], cur, c);
                if (dw < best_w) { best_w = dw; best_pc = upc; }
                break;
            }
            case OP_MESH: {
                const R before = best_w;
                mesh_closest<R, STATS>(sc, sc.meshes[arg], sc.mesh_bounds[arg], tb.tri_order, cur, tb.chain_scale[chain], stack, stride, levels,
                                       best_w, best_tri, n_nodes, n_tris);
                if (best_w < before) best_pc = upc;
                break;
            }
            default:  // OP_BOUNDS: never used for culling; OP_GROUP: the op form behind it is walked; OP_SKY / OP_SUN: no candidates
                break;
        }
    }
    RtPointHit h;
    h.distance = double(Lim<double>::inf());
    for (int k = 0; k < 3; k++) { h.pos[k] = 0.0; h.normal[k] = 0.0; }
    h.material = -1; h.node = -1; h.prim = -1;
    h.flags = 0u;
    h._reserved = 0ull;
    if (best_pc >= 0) {
        // the winner once more, for its point and normal: same routine on the same operands, so the same distance
        const Op op = sc.ops[best_pc];
        const V3<R> q = point_in_chain(sc, wq, op.chain);
        V3<R> pos, normal;
        int32_t material;
        switch (op.type) {
            case OP_SPHERE: {
                const SpherePrim<R>& s = sc.spheres[op.arg];
                (void)closest_on_sphere(s, q, pos, normal);
                material = s.material;
                break;
            }
            case OP_PLANE: {
                const PlanePrim<R>& p = sc.planes[op.arg];
                (void)closest_on_plane_prim(p, q, pos);
                normal = ld3(p.normal);
                material = p.material;
                break;
            }
            default: {  // OP_MESH
                const TriRec<R>& tr = sc.tris[best_tri];
                (void)closest_on_triangle(ld3(tr.v0), ld3(tr.e1), ld3(tr.e2), q, pos);
                normal = cross(ld3(tr.e1), ld3(tr.e2));
                material = sc.meshes[op.arg].material;
                h.prim = int32_t(tb.tri_order[best_tri]);
                break;
            }
        }
        // to world space as k_rq_resolve takes positions and normals there, innermost transform first; a zero normal (zero-area
        // triangle) stays zero
        const bool has_normal = length_squared(normal) > R(0);
        if (has_normal) normal = to_unit(normal);
        const int32_t b = sc.chain_offsets[op.chain], e = sc.chain_offsets[op.chain + 1];
        for (int32_t k = e - 1; k >= b; k--) {
            const Xform<R>& x = sc.xforms[sc.chain_items[k]];
            pos = xform_apply(x.m, pos, R(1));
            if (has_normal) normal = to_unit(xform_apply(x.m, normal, R(0)));
        }
        if (!has_normal) normal = mk<R>(0, 0, 0);
        uint32_t flags = RT_POINT_FOUND;
        if (dot(wq - pos, normal) < R(0)) flags |= RT_POINT_BACK_SIDE;
        h.distance = double(best_w);
        h.pos[0] = double(pos.x); h.pos[1] = double(pos.y); h.pos[2] = double(pos.z);
        h.normal[0] = double(normal.x); h.normal[1] = double(normal.y); h.normal[2] = double(normal.z);
        h.material = material;
        h.node = tb.op_node[best_pc];
        h.flags = flags;
    }
    out[i] = h;
    if constexpr (STATS) {
        counts[2 * size_t(i)] = n_nodes;
        counts[2 * size_t(i) + 1] = n_tris;
    }
}

// ---------------------------------------------------------------------------------------------
template <typename R>
hipError_t pq_closest_launch(const SceneView<R>& sc, const PqTables<R>& tb, const double* d_points, const double* d_max_distance, uint32_t n,
                             int stack_levels, RtPointHit* d_out, uint32_t* d_counts, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (stack_levels < 1 || stack_levels > kPqMaxStackLevels) return hipErrorInvalidValue;
    const uint32_t lanes = stack_levels <= 32 ? 256u : 128u;
    const size_t lds = size_t(stack_levels) * lanes * sizeof(uint2);
    const dim3 grid((n + lanes - 1u) / lanes), block(lanes);
    if (d_counts)
        hipLaunchKernelGGL((k_pq_closest<R, true>), grid, block, lds, stream, sc, tb, d_points, d_max_distance, n, stack_levels, d_out, d_counts);
    else
        hipLaunchKernelGGL((k_pq_closest<R, false>), grid, block, lds, stream, sc, tb, d_points, d_max_distance, n, stack_levels, d_out, d_counts);
    return hipGetLastError();
}

template hipError_t pq_closest_launch<double>(const SceneView<double>&, const PqTables<double>&, const double*, const double*, uint32_t, int,
                                              RtPointHit*, uint32_t*, hipStream_t);
template hipError_t pq_closest_launch<float>(const SceneView<float>&, const PqTables<float>&, const double*, const double*, uint32_t, int,
                                             RtPointHit*, uint32_t*, hipStream_t);

}  // namespace rt
