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
// Behind the kernels and their launchers: the host side (the scene's lightmap workspace, the stages of rt_bake_lightmap) and
// the entry points rt_lightmap_* and rt_bake_lightmap*.
#include <string.h>  // before rocprim: its texture iterator calls ::memset on the host

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "rt_bake.h"
#include "rt_lightmap.h"
#include "rt_scene_host.h"

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

// ---------------------------------------------------------------------------------------------
// Host side: the lightmap workspace of a scene (RtScene::Lightmap, rt_scene_host.h), the stages of a bake and the entry points
// ---------------------------------------------------------------------------------------------
// (triangle, tile) references a rasterisation may make: RT_LIGHTMAP_MAX_REFS, read at each call; the offsets are 32-bit
static uint64_t lm_max_refs() {
    uint64_t cap = 1ull << 28;
    if (const char* e = std::getenv("RT_LIGHTMAP_MAX_REFS")) cap = std::strtoull(e, nullptr, 10);
    return std::min<uint64_t>(cap, 1ull << 31);
}

// Rasterises `mesh` on `stream` into the buffers that outputs(&d_hits, &d_counts) names (d_counts may come back NULL); returns
// after the kernels.  outputs() runs once the reference count has passed its cap: before that nothing is written or allocated
// but the two totals and the events.
template <typename Outputs>
static int lm_rasterise(RtScene* s, rt::DeviceScene<double>& ds, const rt::LmMeshRef& mesh, uint32_t w, uint32_t h, Outputs&& outputs,
                        hipStream_t stream, const char* who) {
    using namespace rt;
    RtScene::Lightmap& L = s->lm;
    if (int st = rq_tables(s, stream)) return st;
    if (int st = L.totals.reserve(2 * sizeof(unsigned long long))) return st;
    for (Event& e : L.ev)
        if (int st = e.ensure()) return st;
    const TriAttr<double>* attrs = ds.view.attrs;
    HIP_TRY(lm_count_refs_launch(attrs, mesh, w, h, L.totals, stream));
    unsigned long long tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, L.totals, sizeof tot, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t cap = lm_max_refs();
    if (tot[0] > cap)
        return set_err(RT_E_UNSUPPORTED, std::string(who) + ": the map needs " + std::to_string(tot[0]) + " (triangle, tile) references, RT_LIGHTMAP_MAX_REFS allows " +
                                             std::to_string(cap));
    RtRayHit* d_hits = nullptr;
    uint32_t* d_counts = nullptr;
    if (int st = outputs(&d_hits, &d_counts)) return st;
    const uint32_t n_tiles = ((w + kLmTile - 1u) / kLmTile) * ((h + kLmTile - 1u) / kLmTile);
    size_t scan_bytes = 0;
    HIP_TRY(lm_scan_temp_bytes(n_tiles + 1u, &scan_bytes));
    if (int st = L.tile_count.reserve((size_t(n_tiles) + 1) * 4)) return st;
    if (int st = L.tile_offset.reserve((size_t(n_tiles) + 1) * 4)) return st;
    if (int st = L.tile_cursor.reserve(size_t(n_tiles) * 4)) return st;
    if (int st = L.refs.reserve(std::max<size_t>(1, size_t(tot[0])) * 4, "the lightmap's tile references do not fit in device memory (RT_LIGHTMAP_MAX_REFS caps them)")) return st;
    if (int st = L.scan_temp.reserve(std::max<size_t>(16, scan_bytes))) return st;
    const LmWorkspace ws{L.tile_count, L.tile_offset, L.tile_cursor, L.refs, L.totals, L.scan_temp.get(), scan_bytes};
    HIP_TRY(hipEventRecord(L.ev[0], stream));
    HIP_TRY(lm_bin_launch(attrs, mesh, w, h, ws, stream));
    HIP_TRY(hipEventRecord(L.ev[1], stream));
    HIP_TRY(lm_raster_launch(ds.view, s->rq.tri_order, mesh, w, h, ws, d_hits, d_counts, stream));
    HIP_TRY(hipEventRecord(L.ev[2], stream));
    HIP_TRY(hipMemcpyAsync(tot, L.totals, sizeof tot, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float bin_ms = 0.f, raster_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&bin_ms, L.ev[0], L.ev[1]));
    HIP_TRY(hipEventElapsedTime(&raster_ms, L.ev[1], L.ev[2]));
    L.stats = RtLightmapStats{};
    L.stats.bin_ms = bin_ms;
    L.stats.raster_ms = raster_ms;
    L.stats.texels = uint64_t(w) * h;
    L.stats.covered_texels = tot[1];
    L.stats.tile_refs = tot[0];
    L.stats.width = w;
    L.stats.height = h;
    return RT_OK;
}

// The scene's f64 tables (built as the first f64 query would), then run(tables).
template <typename F>
static int lm_with_f64(RtScene* s, F&& run) {
    using namespace rt;
    HIP_TRY(hipSetDevice(s->device));
    return with_tables(s, RT_PRECISION_F64, [&](auto& ds) -> int {
        if constexpr (std::is_same_v<typename std::decay_t<decltype(ds)>::Real, double>) return run(ds);
        else return set_err(RT_E_INVALID, "lightmaps are f64");
    });
}

static int lightmap_texels_impl(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t w, uint32_t h, RtRayHit* hits, uint32_t* counts, bool host,
                                void* stream, const char* who) {
    using namespace rt;
    if (!scene) return set_err(RT_E_INVALID, std::string(who) + ": scene is NULL");
    if (!hits) return set_err(RT_E_INVALID, std::string(who) + ": hits_out is NULL");
    LmMeshRef mesh;
    if (int st = lightmap_select(scene->held.d, scene->compiled, node, instance, w, h, who, &mesh)) return st;
    RtScene* s = const_cast<RtScene*>(scene);  // workspace + lazily built tables; the scene data itself is immutable
    const size_t n = size_t(w) * h;
    return lm_with_f64(s, [&](DeviceScene<double>& ds) -> int {
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(s->stream);
        RtScene::Lightmap& L = s->lm;
        auto outputs = [&](RtRayHit** d_hits, uint32_t** d_counts) -> int {
            if (!host) { *d_hits = hits; *d_counts = counts; return RT_OK; }
            if (int r = L.hits.reserve(n * sizeof(RtRayHit))) return r;
            if (counts)
                if (int r = L.counts.reserve(n * 4)) return r;
            *d_hits = L.hits;
            *d_counts = counts ? L.counts.get() : nullptr;
            return RT_OK;
        };
        if (int r = lm_rasterise(s, ds, mesh, w, h, outputs, st, who)) return r;
        if (!host) return RT_OK;
        HIP_TRY(hipMemcpy(hits, L.hits, n * sizeof(RtRayHit), hipMemcpyDeviceToHost));
        if (counts) HIP_TRY(hipMemcpy(counts, L.counts, n * 4, hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

// `passes` dilation passes from (rgba, cov) to (rgba_out, cov_out), ping-pong through the two scratch pairs, which are read only
// when passes > 1.  None of the six may be another of them.  Enqueues only.
static int lm_dilate_enqueue(const double* rgba, const uint8_t* cov, uint32_t w, uint32_t h, int32_t passes, double* rgba_out, uint8_t* cov_out,
                             double* rgba_tmp, uint8_t* cov_tmp, hipStream_t stream) {
    using namespace rt;
    const size_t n = size_t(w) * h;
    if (passes == 0) {
        HIP_TRY(hipMemcpyAsync(rgba_out, rgba, n * 32, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(lm_coverage_bytes_launch(cov, n, cov_out, stream));
        return RT_OK;
    }
    const double* src = rgba;
    const uint8_t* src_c = cov;
    for (int32_t k = 1; k <= passes; k++) {
        const bool to_out = ((passes - k) % 2) == 0;
        double* dst = to_out ? rgba_out : rgba_tmp;
        uint8_t* dst_c = to_out ? cov_out : cov_tmp;
        HIP_TRY(lm_dilate_launch(src, src_c, w, h, dst, dst_c, stream));
        src = dst;
        src_c = dst_c;
    }
    return RT_OK;
}

static int lm_dilate_check(const void* a, const void* b, const void* c, const void* d, uint32_t w, uint32_t h, int32_t passes, const char* who) {
    using namespace rt;
    const std::string p = std::string(who) + ": ";
    if (!a) return set_err(RT_E_INVALID, p + "rgba is NULL");
    if (!b) return set_err(RT_E_INVALID, p + "coverage is NULL");
    if (!c) return set_err(RT_E_INVALID, p + "rgba_out is NULL");
    if (!d) return set_err(RT_E_INVALID, p + "coverage_out is NULL");
    if (w == 0 || w > kLmMaxDim) return set_err(RT_E_INVALID, p + "w must be in 1 .. 16384");
    if (h == 0 || h > kLmMaxDim) return set_err(RT_E_INVALID, p + "h must be in 1 .. 16384");
    if (passes < 0) return set_err(RT_E_INVALID, p + "passes must not be negative");
    if (a == c || b == d) return set_err(RT_E_INVALID, p + "the outputs must not be the inputs");
    return RT_OK;
}

static int bake_lightmap_impl(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t w, uint32_t h, uint32_t kind, const RtRenderParams* rp,
                              const RtBakeParams* bp, int32_t passes, double* rgba_out, uint8_t* cov_out, bool host, void* stream, const char* who) {
    using namespace rt;
    const std::string p = std::string(who) + ": ";
    if (!scene) return set_err(RT_E_INVALID, p + "scene is NULL");
    if (!rgba_out) return set_err(RT_E_INVALID, p + "rgba_out is NULL");
    if (!cov_out) return set_err(RT_E_INVALID, p + "coverage_out is NULL");
    if (kind != RT_LIGHTMAP_IRRADIANCE && kind != RT_LIGHTMAP_VISIBILITY) return set_err(RT_E_INVALID, p + "kind must be RT_LIGHTMAP_IRRADIANCE or RT_LIGHTMAP_VISIBILITY");
    if (passes < 0) return set_err(RT_E_INVALID, p + "dilate_passes must not be negative");
    LmMeshRef mesh;
    if (int st = lightmap_select(scene->held.d, scene->compiled, node, instance, w, h, who, &mesh)) return st;
    if (!scene->compiled.volumes.empty()) return set_err(RT_E_UNSUPPORTED, p + "a scene with volumes has no hit-record bakes");
    const size_t n = size_t(w) * h;
    if (kind == RT_LIGHTMAP_IRRADIANCE) {  // what the bake would refuse, before the device is touched
        const TableCall c{who, {scene, "hits", sizeof(RtRayHit)}, {}, "rgba_out", 32, "point table", "point"};
        if (int st = table_render_check(scene, n, rp, rgba_out, c)) return st;
    } else if (bp) {  // the visibility bake's rules
        if (bp->precision != RT_PRECISION_F64 && bp->precision != RT_PRECISION_F32) return set_err(RT_E_INVALID, p + "precision must be RT_PRECISION_F64 or RT_PRECISION_F32");
        if (int st = bake_params_check(*bp, p)) return st;
    }
    RtScene* s = const_cast<RtScene*>(scene);  // workspace + lazily built tables; the scene data itself is immutable
    return lm_with_f64(s, [&](DeviceScene<double>& ds) -> int {
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(s->stream);
        RtScene::Lightmap& L = s->lm;
        auto outputs = [&](RtRayHit** d_hits, uint32_t** d_counts) -> int {  // the stages' buffers, once the rasteriser has not refused
            if (int r = L.hits.reserve(n * sizeof(RtRayHit))) return r;
            if (int r = L.rgba_a.reserve(n * 32)) return r;
            if (int r = L.cov_a.reserve(n)) return r;
            if (int r = L.cov_b.reserve(n)) return r;
            if (passes > 1) {
                if (int r = L.rgba_b.reserve(n * 32)) return r;
                if (int r = L.cov_c.reserve(n)) return r;
            }
            if (host)
                if (int r = L.rgba_o.reserve(n * 32)) return r;
            *d_hits = L.hits;
            *d_counts = nullptr;
            return RT_OK;
        };
        if (int r = lm_rasterise(s, ds, mesh, w, h, outputs, st, who)) return r;
        HIP_TRY(lm_coverage_launch(L.hits, n, L.cov_a, st));
        if (kind == RT_LIGHTMAP_IRRADIANCE) {
            if (int r = rt_bake_irradiance_hits_device(scene, n, L.hits, rp, L.rgba_a, st)) return r;
        } else {
            if (int r = L.vis.reserve(n * sizeof(RtBakeResult))) return r;
            if (int r = rt_bake_visibility_hits_device(scene, n, L.hits, bp, L.vis, st)) return r;
            HIP_TRY(lm_visibility_rgba_launch(L.vis, L.cov_a, n, L.rgba_a, st));
        }
        double* d_rgba = host ? L.rgba_o.get() : rgba_out;
        if (int r = lm_dilate_enqueue(L.rgba_a, L.cov_a, w, h, passes, d_rgba, L.cov_b, L.rgba_b, L.cov_c, st)) return r;
        if (host) {
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(hipMemcpy(rgba_out, L.rgba_o, n * 32, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cov_out, L.cov_a, n, hipMemcpyDeviceToHost));
        } else {
            HIP_TRY(hipMemcpyAsync(cov_out, L.cov_a, n, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return RT_OK;
    });
}

extern "C" {

int rt_lightmap_texels(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* hits_out,
                       uint32_t* counts_out_or_null) {
    return lightmap_texels_impl(scene, node, instance, width, height, hits_out, counts_out_or_null, true, nullptr, "rt_lightmap_texels");
}
int rt_lightmap_texels_device(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* d_hits_out,
                              uint32_t* d_counts_out_or_null, void* stream) {
    return lightmap_texels_impl(scene, node, instance, width, height, d_hits_out, d_counts_out_or_null, false, stream, "rt_lightmap_texels_device");
}
int rt_lightmap_stats(const RtScene* scene, RtLightmapStats* out) {
    if (!scene || !out) return rt::set_err(RT_E_INVALID, "rt_lightmap_stats: NULL argument");
    *out = scene->lm.stats;
    return RT_OK;
}

int rt_lightmap_dilate_device(int device, const double* d_rgba, const uint8_t* d_coverage, uint32_t w, uint32_t h, int32_t passes,
                              double* d_rgba_out, uint8_t* d_coverage_out, void* stream) {
    using namespace rt;
    if (int st = lm_dilate_check(d_rgba, d_coverage, d_rgba_out, d_coverage_out, w, h, passes, "rt_lightmap_dilate_device")) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = size_t(w) * h;
    DevBuf<double> tmp;
    DevBuf<uint8_t> tmp_c;
    if (passes > 1) {
        if (int st = tmp.reserve(n * 32)) return st;
        if (int st = tmp_c.reserve(n)) return st;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int r = lm_dilate_enqueue(d_rgba, d_coverage, w, h, passes, d_rgba_out, d_coverage_out, tmp, tmp_c, st)) return r;
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_lightmap_dilate(int device, const double* rgba, const uint8_t* coverage, uint32_t w, uint32_t h, int32_t passes, double* rgba_out,
                       uint8_t* coverage_out) {
    using namespace rt;
    if (int st = lm_dilate_check(rgba, coverage, rgba_out, coverage_out, w, h, passes, "rt_lightmap_dilate")) return st;
    HIP_TRY(hipSetDevice(device));
    const size_t n = size_t(w) * h;
    DevBuf<double> in, out;
    DevBuf<uint8_t> in_c, out_c;
    if (int st = in.reserve(n * 32)) return st;
    if (int st = out.reserve(n * 32)) return st;
    if (int st = in_c.reserve(n)) return st;
    if (int st = out_c.reserve(n)) return st;
    HIP_TRY(hipMemcpy(in, rgba, n * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in_c, coverage, n, hipMemcpyHostToDevice));
    if (int st = rt_lightmap_dilate_device(device, in, in_c, w, h, passes, out, out_c, nullptr)) return st;
    HIP_TRY(hipMemcpy(rgba_out, out, n * 32, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(coverage_out, out_c, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_bake_lightmap(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, uint32_t kind,
                     const RtRenderParams* render_params, const RtBakeParams* bake_params, int32_t dilate_passes, double* rgba_out,
                     uint8_t* coverage_out) {
    return bake_lightmap_impl(scene, node, instance, width, height, kind, render_params, bake_params, dilate_passes, rgba_out, coverage_out, true, nullptr,
                              "rt_bake_lightmap");
}
int rt_bake_lightmap_device(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, uint32_t kind,
                            const RtRenderParams* render_params, const RtBakeParams* bake_params, int32_t dilate_passes, double* d_rgba_out,
                            uint8_t* d_coverage_out, void* stream) {
    return bake_lightmap_impl(scene, node, instance, width, height, kind, render_params, bake_params, dilate_passes, d_rgba_out, d_coverage_out, false, stream,
                              "rt_bake_lightmap_device");
}

}  // extern "C"
