// rt_point.hip — point queries: the closest surface point of the scene to points the caller supplies (include/rt_mi355.h:
// rt_closest_points).  A translation unit of its own: no other kernel is touched.
//   k_pq_closest: one lane per point walks the op form of the scene program without ever skipping (the reference's boxes are
//   not all correct, SURVEY B-8, so they cannot cull by distance); spheres and parallelograms run their exact tests, a mesh
//   op is searched nearest child first by mesh_closest (rt_point.h) with a radius that shrinks as candidates are found.
// Behind the kernel and its launcher: the host side (per-chain scales, chunk loop) and the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "rt_device.h"
#include "rt_point.h"
#include "rt_scene_host.h"

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

// ---------------------------------------------------------------------------------------------
// Host side: the point-query workspace of a scene (RtScene::Points, rt_scene_host.h), the chunk loop and the entry points
// ---------------------------------------------------------------------------------------------
// Host only, f64: scale[c] = s of the composed linear part L of chain c (object -> world, outermost transform first),
// s^2 = tr(L^T L) / 3.  False, with the reason in `why`, if the chain over a sphere, plane or mesh op is not a similarity:
// max |L^T L - s^2 I| <= 1e-9 s^2 is one.
static bool pq_chain_scales(const CompiledScene& cs, std::vector<double>& scale, std::string& why) {
    const size_t n_chains = cs.chain_offsets.empty() ? 0 : cs.chain_offsets.size() - 1;
    scale.assign(std::max<size_t>(1, n_chains), 1.0);
    std::vector<char> similar(scale.size(), 1);
    for (size_t c = 0; c < n_chains; c++) {
        double L[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int32_t k = cs.chain_offsets[c]; k < cs.chain_offsets[c + 1]; k++) {
            const double* m = cs.xforms[size_t(cs.chain_items[size_t(k)])].m;
            double P[9];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) P[3 * i + j] = L[3 * i] * m[j] + L[3 * i + 1] * m[4 + j] + L[3 * i + 2] * m[8 + j];
            std::copy(P, P + 9, L);
        }
        double G[9];  // L^T L
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) G[3 * i + j] = L[i] * L[j] + L[3 + i] * L[3 + j] + L[6 + i] * L[6 + j];
        const double s2 = (G[0] + G[4] + G[8]) / 3.0;
        double dev = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) dev = std::fmax(dev, std::fabs(G[3 * i + j] - (i == j ? s2 : 0.0)));
        similar[c] = (s2 > 0.0 && std::isfinite(s2) && dev <= 1e-9 * s2) ? 1 : 0;
        scale[c] = std::sqrt(s2);
    }
    for (size_t pc = 0; pc < cs.ops.size(); pc++) {
        const Op& op = cs.ops[pc];
        if ((op.type == OP_SPHERE || op.type == OP_PLANE || op.type == OP_MESH) && !similar[size_t(op.chain)]) {
            why = "the transforms over node " + std::to_string(pc < cs.op_node.size() ? cs.op_node[pc] : -1) +
                  " do not compose to a similarity (non-uniform scale or shear): object-space distances are not world distances";
            return false;
        }
    }
    return true;
}

// n points in chunks.  counts != NULL: the counting variant, `out` is then unused and the records go to a buffer of this call.
template <typename R>
int closest_points_typed(RtScene* s, DeviceScene<R>& ds, uint64_t n, const double* points, const double* max_distance, RtPointHit* out,
                         uint32_t* counts, const std::vector<double>& scale, int levels, bool host, hipStream_t stream) {
    RtScene::Points& pw = s->points;
    const uint32_t precision = sizeof(R) == 8 ? RT_PRECISION_F64 : RT_PRECISION_F32;
    if (int st = rq_tables(s, stream)) return st;
    if (!pw.chain_scale || pw.scale_generation != s->generation || pw.scale_precision != precision) {
        std::vector<R> rounded(scale.begin(), scale.end());
        if (int st = pw.chain_scale.reserve(rounded.size() * sizeof(R))) return st;
        HIP_TRY(hipMemcpyAsync(pw.chain_scale, rounded.data(), rounded.size() * sizeof(R), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        pw.scale_generation = s->generation;
        pw.scale_precision = precision;
    }
    const PqTables<R> tb{s->rq.op_node, s->rq.tri_order, reinterpret_cast<const R*>(pw.chain_scale.get())};
    const uint32_t chunk = rq_chunk();
    DevBuf<RtPointHit> records;  // counting variant only
    if (counts)
        if (int st = records.reserve(size_t(std::min<uint64_t>(n, chunk)) * sizeof(RtPointHit))) return st;
    ChunkTimes t;
    auto launch = [&](uint64_t, uint32_t m, const void* const* d_in, void* d_out) -> int {
        HIP_TRY(pq_closest_launch<R>(ds.view, tb, static_cast<const double*>(d_in[0]), static_cast<const double*>(d_in[1]), m, levels,
                                     counts ? records.get() : static_cast<RtPointHit*>(d_out), counts ? static_cast<uint32_t*>(d_out) : nullptr, stream));
        return RT_OK;
    };
    void* const dst = counts ? static_cast<void*>(counts) : static_cast<void*>(out);
    if (int st = run_chunks(pw.stage, n, chunk, host, {{points, 24}, {max_distance, 8}}, dst, counts ? 8 : sizeof(RtPointHit), stream, launch, &t)) return st;
    if (!counts) record_query_stats<R>(pw.stats, t, n);
    return RT_OK;
}

}  // namespace rt

extern "C" {

// Every refusal is decided here, on the host, before the tables of `precision` or any workspace exist.
static int closest_points_impl(const RtScene* scene, uint64_t n, const double* points, const double* max_distance, uint32_t precision,
                               RtPointHit* out, uint32_t* counts, bool host, void* stream, const char* who) {
    using namespace rt;
    if (!scene) return set_err(RT_E_INVALID, std::string(who) + ": NULL scene");
    if (precision != RT_PRECISION_F64 && precision != RT_PRECISION_F32) return set_err(RT_E_INVALID, std::string(who) + ": precision must be RT_PRECISION_F64 or RT_PRECISION_F32");
    const CompiledScene& cs = scene->compiled;
    if (!cs.volumes.empty())
        return set_err(RT_E_UNSUPPORTED, std::string(who) + ": point queries do not support scenes with volumes (a medium has no surface to be near)");
    if (n == 0) return RT_OK;
    if (!points || !(counts ? static_cast<const void*>(counts) : static_cast<const void*>(out))) return set_err(RT_E_INVALID, std::string(who) + ": NULL array");
    std::vector<double> scale;
    std::string why;
    if (!pq_chain_scales(cs, scale, why)) return set_err(RT_E_UNSUPPORTED, std::string(who) + ": " + why);
    const int levels = cs.meshes.empty() ? 1 : int(cs.max_bvh4_stack) + 1;
    if (levels > kPqMaxStackLevels) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the point-query kernel's LDS traversal stack");
    RtScene* s = const_cast<RtScene*>(scene);  // workspace + lazily built tables; the scene data itself is immutable
    HIP_TRY(hipSetDevice(s->device));
    return with_tables(s, precision, [&](auto& ds) -> int {
        return closest_points_typed(s, ds, n, points, max_distance, out, counts, scale, levels, host, stream ? static_cast<hipStream_t>(stream) : s->stream);
    });
}

int rt_closest_points(const RtScene* scene, uint64_t n, const double* points, const double* max_distance, uint32_t precision, RtPointHit* out) {
    return closest_points_impl(scene, n, points, max_distance, precision, out, nullptr, true, nullptr, "rt_closest_points");
}
int rt_closest_points_device(const RtScene* scene, uint64_t n, const double* d_points, const double* d_max_distance, uint32_t precision,
                             RtPointHit* d_out, void* stream) {
    return closest_points_impl(scene, n, d_points, d_max_distance, precision, d_out, nullptr, false, stream, "rt_closest_points_device");
}
int rt_debug_closest_points_counts(const RtScene* scene, uint64_t n, const double* points, const double* max_distance, uint32_t precision,
                                   uint32_t* counts_out) {
    return closest_points_impl(scene, n, points, max_distance, precision, nullptr, counts_out, true, nullptr, "rt_debug_closest_points_counts");
}
int rt_point_query_stats(const RtScene* scene, RtRayQueryStats* out) {
    if (!scene || !out) return rt::set_err(RT_E_INVALID, "rt_point_query_stats: NULL argument");
    *out = scene->points.stats;
    return RT_OK;
}

}  // extern "C"
