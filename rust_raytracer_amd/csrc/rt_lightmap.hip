// rt_lightmap.hip — UV-space rasterisation of one mesh op into RtRayHit records, and lightmap dilation.
//
//   1. k_lm_count_refs   per triangle: the rectangle of tiles its UV box can touch (rt_lightmap.h lm_texel_rect); the sum of
//                        the rectangles' sizes, so that the caller can refuse before anything is allocated
//   2. k_lm_bin<false>   per triangle: +1 on every tile of its rectangle            (atomics)
//   3. rocprim exclusive scan of the per-tile counts                                 [library primitive]
//   4. k_lm_bin<true>    per triangle: its leaf slot into every tile's list          (atomics: the ORDER inside a list is
//                        not deterministic and does not matter: the raster takes a minimum and a count)
//   5. k_lm_raster       one 256-lane workgroup per tile of 16 x 16 texels, one lane per texel: the tile's list goes through
//                        LDS in batches of 256 triangles (each lane stages one), every lane walks the batch - all lanes read
//                        the same LDS address, a broadcast - and keeps the lowest covering triangle and the count; then the
//                        record of the winner.
// The 16-texel tile and the 256-triangle batch are first choices from the LDS budget, not measured optima.
// Always f64: a setup step whose records are f64 anyway.
#include <string.h>  // before rocprim: its texture iterator calls ::memset on the host

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "rt_lightmap.h"

namespace rt {

// The triangle of leaf slot `slot` as the rule sees it: false if it covers nothing.
__device__ __forceinline__ bool lm_load_tri(const TriAttr<double>& at, LmUV& a, LmUV& b, LmUV& c, double& area) {
    if (!at.has_uv) return false;
    a = lm_uv(at.uv0); b = lm_uv(at.uv1); c = lm_uv(at.uv2);
    return lm_area(a, b, c, &area) != 0;
}

__device__ __forceinline__ bool lm_tile_rect(const TriAttr<double>& at, uint32_t w, uint32_t h, uint32_t& tx0, uint32_t& tx1, uint32_t& ty0, uint32_t& ty1) {
    LmUV a, b, c;
    double area;
    if (!lm_load_tri(at, a, b, c, area)) return false;
    uint32_t x0, x1, y0, y1;
    if (!lm_texel_rect(a, b, c, area, w, h, &x0, &x1, &y0, &y1)) return false;
    tx0 = x0 / kLmTile; tx1 = x1 / kLmTile; ty0 = y0 / kLmTile; ty1 = y1 / kLmTile;
    return true;
}

__global__ void __launch_bounds__(256) k_lm_count_refs(const TriAttr<double>* __restrict__ attrs, uint32_t n_tris, uint32_t w, uint32_t h,
                                                       unsigned long long* __restrict__ totals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    uint32_t tx0, tx1, ty0, ty1;
    if (!lm_tile_rect(attrs[i], w, h, tx0, tx1, ty0, ty1)) return;
    atomicAdd(&totals[0], (unsigned long long)(tx1 - tx0 + 1u) * (unsigned long long)(ty1 - ty0 + 1u));
}

// FILL = false: counts per tile; FILL = true: the slot into refs[offset[tile] + cursor[tile]++].
template <bool FILL>
__global__ void __launch_bounds__(256) k_lm_bin(const TriAttr<double>* __restrict__ attrs, uint32_t n_tris, uint32_t w, uint32_t h, uint32_t tiles_x,
                                                uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_offset,
                                                uint32_t* __restrict__ tile_cursor, uint32_t* __restrict__ refs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    uint32_t tx0, tx1, ty0, ty1;
    if (!lm_tile_rect(attrs[i], w, h, tx0, tx1, ty0, ty1)) return;
    for (uint32_t ty = ty0; ty <= ty1; ty++)
        for (uint32_t tx = tx0; tx <= tx1; tx++) {
            const uint32_t t = ty * tiles_x + tx;
            if (FILL) {
                const uint32_t k = atomicAdd(&tile_cursor[t], 1u);
                if (k < tile_offset[t + 1] - tile_offset[t]) refs[tile_offset[t] + k] = i;  // always true: same rectangle as the count
            } else {
                atomicAdd(&tile_count[t], 1u);
            }
        }
}

struct LmStaged {
    double uv[kLmBatch][6];
    uint32_t slot[kLmBatch];
    uint32_t index[kLmBatch];  // the triangle in RtMesh.tri_pos order
};

__global__ void __launch_bounds__(256) k_lm_raster(SceneView<double> sc, const uint32_t* __restrict__ tri_order, LmMeshRef mesh, uint32_t w, uint32_t h,
                                                   uint32_t tiles_x, const uint32_t* __restrict__ tile_offset, const uint32_t* __restrict__ refs,
                                                   RtRayHit* __restrict__ hits, uint32_t* __restrict__ counts, unsigned long long* __restrict__ totals) {
    __shared__ LmStaged st;
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const uint32_t x = (tile % tiles_x) * kLmTile + (lane % kLmTile), y = (tile / tiles_x) * kLmTile + (lane / kLmTile);
    const bool inside = x < w && y < h;
    const LmUV p = {lm_centre(x, w), lm_centre(y, h)};
    const uint32_t first = tile_offset[tile], end = tile_offset[tile + 1];
    const TriAttr<double>* attrs = sc.attrs + mesh.tri_base;
    uint32_t best = 0xFFFFFFFFu, best_slot = 0, count = 0;
    double best_area = 0.0, best_wb = 0.0, best_wc = 0.0;
    for (uint32_t base = first; base < end; base += kLmBatch) {
        const uint32_t m = min(kLmBatch, end - base);
        __syncthreads();  // the previous batch has been walked by every lane
        if (lane < m) {
            const uint32_t slot = refs[base + lane];
            const TriAttr<double>& at = attrs[slot];
            st.uv[lane][0] = at.uv0[0]; st.uv[lane][1] = at.uv0[1];
            st.uv[lane][2] = at.uv1[0]; st.uv[lane][3] = at.uv1[1];
            st.uv[lane][4] = at.uv2[0]; st.uv[lane][5] = at.uv2[1];
            st.slot[lane] = slot;
            st.index[lane] = tri_order[mesh.tri_base + slot];
        }
        __syncthreads();
        if (inside) {
            for (uint32_t k = 0; k < m; k++) {
                const LmUV a = {st.uv[k][0], st.uv[k][1]}, b = {st.uv[k][2], st.uv[k][3]}, c = {st.uv[k][4], st.uv[k][5]};
                double area, wb, wc;
                if (lm_covers(a, b, c, p, &area, &wb, &wc)) {
                    count++;
                    const uint32_t id = st.index[k];
                    if (id < best) { best = id; best_slot = st.slot[k]; best_area = area; best_wb = wb; best_wc = wc; }
                }
            }
        }
    }
    if (!inside) return;
    const size_t i = size_t(y) * w + x;
    RtRayHit rec = lm_miss_record();
    if (count != 0u) {
        const uint32_t s = mesh.tri_base + best_slot;
        rec = lm_record(sc.tris[s], sc.attrs[s], mesh.flat != 0u, best_area, best_wb, best_wc, sc.chain_offsets, sc.chain_items, sc.xforms, mesh.chain,
                        mesh.material, mesh.node, int32_t(best));
        atomicAdd(&totals[1], 1ull);
    }
    hits[i] = rec;
    if (counts) counts[i] = count;
}

__global__ void __launch_bounds__(256) k_lm_dilate(const double* __restrict__ rgba, const uint8_t* __restrict__ cov, uint32_t w, uint32_t h,
                                                   double* __restrict__ rgba_out, uint8_t* __restrict__ cov_out) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= size_t(w) * h) return;
    double o[4];
    uint8_t c;
    lm_dilate_texel(rgba, cov, w, h, uint32_t(i % w), uint32_t(i / w), o, &c);
    for (int k = 0; k < 4; k++) rgba_out[4 * i + size_t(k)] = o[k];
    cov_out[i] = c;
}

__global__ void __launch_bounds__(256) k_lm_coverage(const RtRayHit* __restrict__ hits, uint64_t n, uint8_t* __restrict__ cov) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cov[i] = (hits[i].flags & RT_RAY_HIT) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_lm_coverage_bytes(const uint8_t* __restrict__ cov, uint64_t n, uint8_t* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = cov[i] ? 1 : 0;
}

// visibility into (r, g, b), 0 into w; an uncovered texel is zeroed
__global__ void __launch_bounds__(256) k_lm_visibility_rgba(const RtBakeResult* __restrict__ res, const uint8_t* __restrict__ cov, uint64_t n,
                                                            double* __restrict__ rgba) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = cov[i] ? res[i].visibility : 0.0;
    rgba[4 * i] = v; rgba[4 * i + 1] = v; rgba[4 * i + 2] = v; rgba[4 * i + 3] = 0.0;
}

static uint32_t lm_tiles(uint32_t n) { return (n + kLmTile - 1u) / kLmTile; }

hipError_t lm_scan_temp_bytes(uint32_t n, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, size_t(n), rocprim::plus<uint32_t>(),
                                   hipStream_t(0));
}

hipError_t lm_count_refs_launch(const TriAttr<double>* attrs, const LmMeshRef& mesh, uint32_t w, uint32_t h, unsigned long long* totals, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), stream)) return e;
    if (mesh.n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lm_count_refs, dim3((mesh.n_tris + 255u) / 256u), dim3(256), 0, stream, attrs + mesh.tri_base, mesh.n_tris, w, h, totals);
    return hipGetLastError();
}

hipError_t lm_bin_launch(const TriAttr<double>* attrs, const LmMeshRef& mesh, uint32_t w, uint32_t h, const LmWorkspace& ws, hipStream_t stream) {
    const uint32_t tiles_x = lm_tiles(w), n_tiles = tiles_x * lm_tiles(h);
    if (hipError_t e = hipMemsetAsync(ws.tile_count, 0, (size_t(n_tiles) + 1) * 4, stream)) return e;
    if (hipError_t e = hipMemsetAsync(ws.tile_cursor, 0, size_t(n_tiles) * 4, stream)) return e;
    const dim3 grid((mesh.n_tris + 255u) / 256u), block(256);
    if (mesh.n_tris) hipLaunchKernelGGL((k_lm_bin<false>), grid, block, 0, stream, attrs + mesh.tri_base, mesh.n_tris, w, h, tiles_x, ws.tile_count, ws.tile_offset, ws.tile_cursor, ws.refs);
    size_t bytes = ws.scan_temp_bytes;
    if (hipError_t e = rocprim::exclusive_scan(ws.scan_temp, bytes, ws.tile_count, ws.tile_offset, 0u, size_t(n_tiles) + 1, rocprim::plus<uint32_t>(), stream)) return e;
    if (mesh.n_tris) hipLaunchKernelGGL((k_lm_bin<true>), grid, block, 0, stream, attrs + mesh.tri_base, mesh.n_tris, w, h, tiles_x, ws.tile_count, ws.tile_offset, ws.tile_cursor, ws.refs);
    return hipGetLastError();
}

hipError_t lm_raster_launch(const SceneView<double>& sc, const uint32_t* tri_order, const LmMeshRef& mesh, uint32_t w, uint32_t h, const LmWorkspace& ws,
                            RtRayHit* d_hits, uint32_t* d_counts, hipStream_t stream) {
    const uint32_t tiles_x = lm_tiles(w), n_tiles = tiles_x * lm_tiles(h);
    hipLaunchKernelGGL(k_lm_raster, dim3(n_tiles), dim3(256), 0, stream, sc, tri_order, mesh, w, h, tiles_x, ws.tile_offset, ws.refs, d_hits, d_counts, ws.totals);
    return hipGetLastError();
}

hipError_t lm_dilate_launch(const double* d_rgba, const uint8_t* d_cov, uint32_t w, uint32_t h, double* d_rgba_out, uint8_t* d_cov_out, hipStream_t stream) {
    const size_t n = size_t(w) * h;
    hipLaunchKernelGGL(k_lm_dilate, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, d_rgba, d_cov, w, h, d_rgba_out, d_cov_out);
    return hipGetLastError();
}
hipError_t lm_coverage_launch(const RtRayHit* d_hits, uint64_t n, uint8_t* d_cov, hipStream_t stream) {
    hipLaunchKernelGGL(k_lm_coverage, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, d_hits, n, d_cov);
    return hipGetLastError();
}
hipError_t lm_coverage_bytes_launch(const uint8_t* d_cov, uint64_t n, uint8_t* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_lm_coverage_bytes, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, d_cov, n, d_out);
    return hipGetLastError();
}
hipError_t lm_visibility_rgba_launch(const RtBakeResult* d_res, const uint8_t* d_cov, uint64_t n, double* d_rgba, hipStream_t stream) {
    hipLaunchKernelGGL(k_lm_visibility_rgba, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, d_res, d_cov, n, d_rgba);
    return hipGetLastError();
}

}  // namespace rt
