// rt_lightmap.h — UV-space rasterisation of a mesh into surface records (include/rt_mi355.h rt_lightmap_texels).
// The texel rule is written ONCE here and compiled twice: by hipcc into the kernels of rt_lightmap.hip and by the host
// compiler into the brute-force restatement of rt_desc.cpp (rt_lightmap_texels_desc).  Both builds use -ffp-contract=off:
// the rule depends on one rounding per operation.  Plain C++, no HIP type in this file.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/rt_mi355.h"
#include "rt_scene.h"

#if defined(__HIPCC__)
#define RT_LM_FN __host__ __device__ inline
#else
#define RT_LM_FN inline
#endif

namespace rt {

// Texels per tile side and triangles per LDS batch of the raster kernel.  First choices from the LDS budget (a batch is
// 256 x 56 B = 14 KB), not measured optima.
constexpr uint32_t kLmTile = 16;
constexpr uint32_t kLmBatch = 256;
constexpr uint32_t kLmMaxDim = 16384;

struct LmUV {
    double u, v;
};

// Centre of texel x of a row of n: no flip, row 0 is v near 0 (the addressing of texture/image.rs:40-52).
RT_LM_FN double lm_centre(uint32_t x, uint32_t n) { return (double(x) + 0.5) / double(n); }

RT_LM_FN double lm_edge(LmUV s, LmUV t, LmUV q) { return (t.u - s.u) * (q.v - s.v) - (t.v - s.v) * (q.u - s.u); }
// The edge function of the edge's canonical direction: two triangles that share an edge see exactly opposite values.
RT_LM_FN double lm_cedge(LmUV s, LmUV t, LmUV q) {
    const bool ordered = s.u < t.u || (s.u == t.u && s.v <= t.v);
    return ordered ? lm_edge(s, t, q) : -lm_edge(t, s, q);
}

// The area term A of a triangle: *area = |A|; returns +1 / -1 for A > 0 / A < 0 and 0 for a zero or NaN area, with which
// the triangle covers nothing.
RT_LM_FN int lm_area(LmUV a, LmUV b, LmUV c, double* area) {
    const double A = lm_cedge(a, b, c);
    *area = A < 0.0 ? -A : A;
    return A > 0.0 ? 1 : (A < 0.0 ? -1 : 0);
}

// Does the triangle (a, b, c) cover the centre p?  On true: *area = |A|, *wb, *wc the edge values of b and c with A's sign
// taken out (bu = wb / area, bv = wc / area).
RT_LM_FN bool lm_covers(LmUV a, LmUV b, LmUV c, LmUV p, double* area, double* wb, double* wc) {
    double A = lm_cedge(a, b, c);
    double w_a = lm_cedge(b, c, p), w_b = lm_cedge(c, a, p), w_c = lm_cedge(a, b, p);
    if (A < 0.0) { A = -A; w_a = -w_a; w_b = -w_b; w_c = -w_c; }
    if (!(A > 0.0)) return false;
    if (!(w_a >= 0.0 && w_b >= 0.0 && w_c >= 0.0)) return false;
    *area = A;
    *wb = w_b;
    *wc = w_c;
    return true;
}

// The rectangle of TEXELS [x0, x1] x [y0, y1] (inclusive) that holds every centre the rule can accept for the triangle; false
// if there is none.  The UV box is widened by `slack` in UV units and then by one texel:
//   * a centre the rule accepts has true edge values >= -e with e <= 8 eps L D (L: longest edge, D: farthest vertex from the
//     centre; both <= 4 M with M = max(1, largest |coordinate|)), so it lies outside the box by at most
//     3 e / A * extent <= 1024 eps M^2 / A * extent = slack: far below a texel unless the triangle is a sliver whose area is
//     near the rounding of its own edge functions, and then the box simply grows;
//   * the one texel covers the roundings of the rectangle's own arithmetic (a few ulps of a value below 2^15).
// Anything not finite gives the whole map: conservative, never wrong.
RT_LM_FN bool lm_texel_rect(LmUV a, LmUV b, LmUV c, double area, uint32_t w, uint32_t h, uint32_t* x0, uint32_t* x1, uint32_t* y0, uint32_t* y1) {
    const double ulo = fmin(a.u, fmin(b.u, c.u)), uhi = fmax(a.u, fmax(b.u, c.u));
    const double vlo = fmin(a.v, fmin(b.v, c.v)), vhi = fmax(a.v, fmax(b.v, c.v));
    const double m = fmax(1.0, fmax(fmax(fabs(ulo), fabs(uhi)), fmax(fabs(vlo), fabs(vhi))));
    const double k = 1024.0 * 2.220446049250313e-16 * m * m / area;
    const double su = k * (uhi - ulo), sv = k * (vhi - vlo);
    double fx0 = floor((ulo - su) * double(w) - 0.5) - 1.0, fx1 = ceil((uhi + su) * double(w) - 0.5) + 1.0;
    double fy0 = floor((vlo - sv) * double(h) - 0.5) - 1.0, fy1 = ceil((vhi + sv) * double(h) - 0.5) + 1.0;
    if (!(fx0 >= 0.0)) fx0 = 0.0;  // also NaN
    if (!(fy0 >= 0.0)) fy0 = 0.0;
    if (!(fx1 <= double(w - 1))) fx1 = double(w - 1);
    if (!(fy1 <= double(h - 1))) fy1 = double(h - 1);
    if (fx0 > fx1 || fy0 > fy1) return false;
    *x0 = uint32_t(fx0); *x1 = uint32_t(fx1); *y0 = uint32_t(fy0); *y1 = uint32_t(fy1);
    return true;
}

struct LmV3 {
    double x, y, z;
};
RT_LM_FN LmV3 lm_unit(LmV3 a) {  // vec4.rs:122
    const double len = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return {a.x / len, a.y / len, a.z / len};
}
RT_LM_FN LmV3 lm_apply(const double* m, LmV3 v, double w) {  // mat4.rs:342-353, as xform_apply (rt_device.h)
    return {m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3] * w, m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7] * w,
            m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11] * w};
}

RT_LM_FN RtRayHit lm_miss_record() {
    RtRayHit h;
    h.t = __builtin_huge_val();
    for (int k = 0; k < 3; k++) { h.pos[k] = 0.0; h.normal[k] = 0.0; }
    h.u = 0.0; h.v = 0.0;
    h.material = -1; h.node = -1; h.prim = -1;
    h.flags = 0u;
    h._reserved = 0ull;
    return h;
}

// The record of a covered texel, in the order of mesh.rs:104-147 and Transform::test (transform.rs:132-133).
RT_LM_FN RtRayHit lm_record(const TriRec<double>& tr, const TriAttr<double>& at, bool flat, double area, double wb, double wc,
                            const int32_t* chain_offsets, const int32_t* chain_items, const Xform<double>* xforms, int32_t chain,
                            int32_t material, int32_t node, int32_t prim) {
    const double bu = wb / area, bv = wc / area, bw = 1.0 - bu - bv;
    LmV3 pos = {tr.v0[0] + (tr.e1[0] * bu + tr.e2[0] * bv), tr.v0[1] + (tr.e1[1] * bu + tr.e2[1] * bv), tr.v0[2] + (tr.e1[2] * bu + tr.e2[2] * bv)};
    LmV3 normal;
    if (flat) {
        normal = lm_unit({tr.e1[1] * tr.e2[2] - tr.e1[2] * tr.e2[1], tr.e1[2] * tr.e2[0] - tr.e1[0] * tr.e2[2], tr.e1[0] * tr.e2[1] - tr.e1[1] * tr.e2[0]});
    } else {
        normal = {at.n0[0] * bw + at.n1[0] * bu + at.n2[0] * bv, at.n0[1] * bw + at.n1[1] * bu + at.n2[1] * bv, at.n0[2] * bw + at.n1[2] * bu + at.n2[2] * bv};
    }
    const int32_t b = chain_offsets[chain], e = chain_offsets[chain + 1];
    for (int32_t k = e - 1; k >= b; k--) {  // innermost first
        const double* m = xforms[chain_items[k]].m;
        pos = lm_apply(m, pos, 1.0);
        normal = lm_unit(lm_apply(m, normal, 0.0));
    }
    if (b == e) normal = lm_unit(normal);
    RtRayHit h;
    h.t = 0.0;
    h.pos[0] = pos.x; h.pos[1] = pos.y; h.pos[2] = pos.z;
    h.normal[0] = normal.x; h.normal[1] = normal.y; h.normal[2] = normal.z;
    h.u = at.uv0[0] * bw + at.uv1[0] * bu + at.uv2[0] * bv;
    h.v = at.uv0[1] * bw + at.uv1[1] * bu + at.uv2[1] * bv;
    h.material = material;
    h.node = node;
    h.prim = prim;
    h.flags = RT_RAY_HIT | RT_RAY_FRONT_FACE;
    h._reserved = 0ull;
    return h;
}

RT_LM_FN LmUV lm_uv(const double* p) { return {p[0], p[1]}; }

// Dilation of one texel (rt_lightmap_dilate): an uncovered texel with covered 8-neighbours takes their mean, summed in the
// order dy = -1 .. 1, dx = -1 .. 1, and counts as covered afterwards.  Texels outside the map are no neighbours.
RT_LM_FN void lm_dilate_texel(const double* rgba, const uint8_t* cov, uint32_t w, uint32_t h, uint32_t x, uint32_t y, double out[4], uint8_t* cov_out) {
    const size_t i = size_t(y) * w + x;
    if (cov[i]) {
        for (int k = 0; k < 4; k++) out[k] = rgba[4 * i + size_t(k)];
        *cov_out = 1;
        return;
    }
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t n = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int64_t xx = int64_t(x) + dx, yy = int64_t(y) + dy;
            if ((dx == 0 && dy == 0) || xx < 0 || yy < 0 || xx >= int64_t(w) || yy >= int64_t(h)) continue;
            const size_t j = size_t(yy) * w + size_t(xx);
            if (!cov[j]) continue;
            for (int k = 0; k < 4; k++) sum[k] = sum[k] + rgba[4 * j + size_t(k)];
            n++;
        }
    if (n == 0) {
        for (int k = 0; k < 4; k++) out[k] = rgba[4 * i + size_t(k)];
        *cov_out = 0;
        return;
    }
    for (int k = 0; k < 4; k++) out[k] = sum[k] / double(n);
    *cov_out = 1;
}

// What the raster stage needs of one mesh op, by value.
struct LmMeshRef {
    uint32_t tri_base, n_tris;   // records in tris / attrs / tri_order
    int32_t chain, material, node;
    uint32_t flat;
};
struct LmTimes {
    float bin_ms, raster_ms;
};

}  // namespace rt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace rt {
// Workspace of the rasteriser: the buffers of RtScene::Lightmap (rt_scene_host.h), reserved by lm_rasterise (rt_lightmap.hip).
struct LmWorkspace {
    uint32_t* tile_count;   // n_tiles + 1
    uint32_t* tile_offset;  // n_tiles + 1 (exclusive scan)
    uint32_t* tile_cursor;  // n_tiles
    uint32_t* refs;         // total references (leaf slots relative to the mesh)
    unsigned long long* totals;  // [0] tile references, [1] covered texels
    void* scan_temp;
    size_t scan_temp_bytes;
};
// Bytes of temporary storage the exclusive scan over n values wants.
hipError_t lm_scan_temp_bytes(uint32_t n, size_t* bytes);
// Pass 1: the number of (triangle, tile) references, into ws.totals[0] (ws.totals zeroed first).  Nothing else is read of ws.
hipError_t lm_count_refs_launch(const TriAttr<double>* attrs, const LmMeshRef& mesh, uint32_t w, uint32_t h, unsigned long long* totals, hipStream_t stream);
// Passes 2-4: per-tile counts, exclusive scan, fill.
hipError_t lm_bin_launch(const TriAttr<double>* attrs, const LmMeshRef& mesh, uint32_t w, uint32_t h, const LmWorkspace& ws, hipStream_t stream);
// One workgroup per tile: w x h records to d_hits, the number of covering triangles to d_counts (may be NULL), the number of
// covered texels added to ws.totals[1].
hipError_t lm_raster_launch(const SceneView<double>& sc, const uint32_t* tri_order, const LmMeshRef& mesh, uint32_t w, uint32_t h, const LmWorkspace& ws,
                            RtRayHit* d_hits, uint32_t* d_counts, hipStream_t stream);
// One dilation pass, and the helpers of rt_bake_lightmap: coverage bytes from records, visibility results into rgba.
hipError_t lm_dilate_launch(const double* d_rgba, const uint8_t* d_cov, uint32_t w, uint32_t h, double* d_rgba_out, uint8_t* d_cov_out, hipStream_t stream);
hipError_t lm_coverage_launch(const RtRayHit* d_hits, uint64_t n, uint8_t* d_cov, hipStream_t stream);
hipError_t lm_coverage_bytes_launch(const uint8_t* d_cov, uint64_t n, uint8_t* d_out, hipStream_t stream);  // 0 / 1
hipError_t lm_visibility_rgba_launch(const RtBakeResult* d_res, const uint8_t* d_cov, uint64_t n, double* d_rgba, hipStream_t stream);
}  // namespace rt
#endif
