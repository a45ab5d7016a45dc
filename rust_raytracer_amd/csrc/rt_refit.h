// rt_refit.h — what the kernels' mesh tables are, as functions of (tree topology, vertex positions).
//
// The reader formats of a mesh BVH (BvhNode<R>, BvhNode4f, BvhNode4q, the back-face cone words) are derived from the exact
// f64 child boxes and the triangle records by the per-node formulas below.  They are written ONCE, __host__ __device__:
// derive_mesh_tables (rt_tables.cpp) and build_mesh_cones (the host builder) and the refit kernels of rt_refit.hip (rt_scene_update)
// call the same functions, compiled with -ffp-contract=off on both sides, in f64 with IEEE operations only (+ - * /
// sqrt, floor / ceil / lround, frexp / ldexp), so the two sides give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_bvh.h"
#include "rt_scene.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>

#include "rt_owned.h"
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rt {

// min / max that pick the same operand on both sides when the two compare equal (-0 and +0) or one is NaN
RT_HD inline double rf_min(double a, double b) { return b < a ? b : a; }
RT_HD inline double rf_max(double a, double b) { return b > a ? b : a; }

RT_HD inline float rf_float_below(float f) {  // nextafterf(f, -inf) for every f that float(x) > x can give
    uint32_t b;
    memcpy(&b, &f, 4);
    if ((b << 1) == 0u) b = 0x80000001u;  // +-0 -> the smallest negative number
    else if (b >> 31) b += 1u;
    else b -= 1u;
    memcpy(&f, &b, 4);
    return f;
}
RT_HD inline float rf_float_above(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    if ((b << 1) == 0u) b = 0x00000001u;
    else if (b >> 31) b -= 1u;
    else b += 1u;
    memcpy(&f, &b, 4);
    return f;
}

template <typename R> RT_HD inline R round_down(double x);
template <typename R> RT_HD inline R round_up(double x);
template <> RT_HD inline double round_down<double>(double x) { return x; }
template <> RT_HD inline double round_up<double>(double x) { return x; }
template <> RT_HD inline float round_down<float>(double x) {
    float f = float(x);
    if (double(f) > x) f = rf_float_below(f);
    return f;
}
template <> RT_HD inline float round_up<float>(double x) {
    float f = float(x);
    if (double(f) < x) f = rf_float_above(f);
    return f;
}

// BvhNode<R>: conservative boxes, outward rounding plus a few ulps so that the slab arithmetic never culls a triangle the
// exact test would hit.
template <typename R> RT_HD inline void rf_pad_box2(double lo, double hi, R* olo, R* ohi) {
    if (!(lo <= hi)) { *olo = R(lo); *ohi = R(hi); return; }  // empty child box
    const double m = std::fmax(std::fabs(lo), std::fabs(hi));
    const double e = 8.0 * double(std::numeric_limits<R>::epsilon()) * std::fmax(m, hi - lo);
    *olo = round_down<R>(lo - e);
    *ohi = round_up<R>(hi + e);
}

// The pad of the 4-wide nodes of a mesh (or primitive group) whose box is (lo, hi): 2^-19 x its largest |coordinate|.
RT_HD inline double rf_pad_of_box(const double* lo, const double* hi) {
    double S = 0.0;
    for (int a = 0; a < 3; a++) S = std::fmax(S, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
    if (!std::isfinite(S)) S = 0.0;
    return S * (1.0 / 524288.0);
}

// BvhNode4f: one plane pair of child k, padded by m and rounded outward.
RT_HD inline void rf_pad_box4f(double lo, double hi, double m, float* olo, float* ohi) {
    if (!(lo <= hi)) { *olo = INFINITY; *ohi = -INFINITY; }
    else { *olo = round_down<float>(lo - m); *ohi = round_up<float>(hi + m); }
}

// BvhNode4q: the padded child boxes (as in BvhNode4f) on a per-node 8-bit grid, rounded outward on the grid.  The cell is
// the smallest power of two with extent / cell <= 255.  False: the node does not fit the grid (coordinates beyond 1e38).
RT_HD inline bool rf_quantise4(const double (*lo)[3], const double (*hi)[3], const int32_t* child, double m, float* org_out, float* cell_out,
                               uint32_t* qlo, uint32_t* qhi) {
    for (int a = 0; a < 3; a++) {
        double flo[4], fhi[4];
        bool real[4];
        double lo_min = INFINITY, hi_max = -INFINITY;
        for (int k = 0; k < 4; k++) {
            real[k] = child[k] != kEmptyChild && lo[k][a] <= hi[k][a];
            if (!real[k]) continue;
            flo[k] = double(round_down<float>(lo[k][a] - m));
            fhi[k] = double(round_up<float>(hi[k][a] + m));
            lo_min = std::fmin(lo_min, flo[k]);
            hi_max = std::fmax(hi_max, fhi[k]);
        }
        const bool any = lo_min <= hi_max && std::isfinite(lo_min) && std::isfinite(hi_max);
        const double org = any ? lo_min : 0.0;  // an f32 value
        const double ext = any ? hi_max - org : 0.0;
        int e = -100;
        if (ext > 0.0) {
            (void)std::frexp(ext / 255.0, &e);  // ext / 255 = f 2^e, f in [1/2, 1): 2^e is the cell or twice the cell
            while (ext / std::ldexp(1.0, e) > 255.0) e++;
            while (e > -100 && ext / std::ldexp(1.0, e - 1) <= 255.0) e--;
            e = e < -100 ? -100 : (e > 120 ? 120 : e);
        }
        const double cell = std::ldexp(1.0, e);
        org_out[a] = float(org);
        cell_out[a] = float(cell);
        qlo[a] = 0;
        qhi[a] = 0;
        for (int k = 0; k < 4; k++) {
            uint32_t ql = 255u, qh = 0u;  // empty child: lo > hi, never entered
            if (any && real[k]) {
                const double l = std::floor((flo[k] - org) / cell), h = std::ceil((fhi[k] - org) / cell);
                const double lc = 255.0 < l ? 255.0 : l, hc = 255.0 < h ? 255.0 : h;  // clamped to [0, 255]
                ql = uint32_t(0.0 < lc ? lc : 0.0);
                qh = uint32_t(0.0 < hc ? hc : 0.0);
                if (!(org + ql * cell <= flo[k] && org + qh * cell >= fhi[k])) return false;  // e > 120: coordinates beyond 1e38
            }
            qlo[a] |= ql << (8 * k);
            qhi[a] |= qh << (8 * k);
        }
    }
    return true;
}

// ---- back-face cones (the argument stands in rt_bvh.cpp) ----
constexpr double kConeDirSlack = 0.00682;   // d_dir
constexpr double kConeSafety = 0.001;       // d_safe
constexpr double kConeMinCos = 0.125;       // c >= 1/8: wider cones cull next to nothing

// The unit normal e1 x e2 of a triangle record, or NaN in out[0..2] if the triangle is ill-conditioned.
RT_HD inline void rf_tri_normal(const double* v0, const double* a, const double* b, const ConeLimits& lim, double* out) {
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    const double la = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double lc = std::sqrt(cx * cx + cy * cy + cz * cz);
    bool ok = std::isfinite(v0[0]) && std::isfinite(v0[1]) && std::isfinite(v0[2]);
    ok = ok && la >= lim.min_edge && la <= lim.max_edge && lb >= lim.min_edge && lb <= lim.max_edge;  // false for NaN
    ok = ok && lc >= lim.sigma * la * lb && lc > 0.0;
    const double kNaN = std::numeric_limits<double>::quiet_NaN();
    out[0] = ok ? cx / lc : kNaN;
    out[1] = ok ? cy / lc : kNaN;
    out[2] = ok ? cz / lc : kNaN;
}

// The word of the cone around `axis` (any length) that holds the normals of the slots [lo, hi), or kNeutralCone.
RT_HD inline uint32_t rf_cone_around(const double* normal, uint32_t lo, uint32_t hi, const double* axis) {
    const double l = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!(l > 0.0) || !std::isfinite(l)) return kNeutralCone;  // NaN: an ill-conditioned triangle below
    int q[3];
    double al = 0.0;
    for (int a = 0; a < 3; a++) { q[a] = int(std::lround(127.0 * axis[a] / l)); al += double(q[a]) * double(q[a]); }
    al = std::sqrt(al);
    if (!(al > 0.0)) return kNeutralCone;
    const double ax = q[0] / al, ay = q[1] / al, az = q[2] / al;
    double c = 1.0;
    for (uint32_t t = lo; t < hi; t++) {
        const double d = ax * normal[3 * size_t(t)] + ay * normal[3 * size_t(t) + 1] + az * normal[3 * size_t(t) + 2];
        c = d < c ? d : c;  // std::min(c, d)
        if (c < kConeMinCos) return kNeutralCone;
    }
    if (!(c >= kConeMinCos)) return kNeutralCone;
    const double s = std::sqrt(std::fmax(0.0, 1.0 - c * c));
    const double w = std::ceil(al * (s + kConeDirSlack + kConeSafety));
    if (!(w >= 1.0 && w <= 127.0)) return kNeutralCone;
    return uint32_t(q[0] & 0xFF) | (uint32_t(q[1] & 0xFF) << 8) | (uint32_t(q[2] & 0xFF) << 16) | (uint32_t(w) << 24);
}

// The cone word of a child over the slots [lo, hi), `count` triangles, the sum of whose normals is `sum`.
RT_HD inline uint32_t rf_cone_word(const double* normal, uint32_t lo, uint32_t hi, uint32_t count, const double* sum) {
    if (count == 0 || hi - lo != count) return kNeutralCone;
    uint32_t word = rf_cone_around(normal, lo, hi, sum);
    if (word == kNeutralCone && count >= 2 && count <= 8 && std::isfinite(sum[0])) {
        // A leaf over a fold: the sum leans towards the side with more triangles and loses the other one.  The bisector
        // of the two normals farthest apart is the axis of the narrowest cone that holds those two.
        uint32_t bi = lo, bj = lo;
        double least = 2.0;
        for (uint32_t i = lo; i < hi; i++)
            for (uint32_t j = i + 1; j < hi; j++) {
                const double* ni = &normal[3 * size_t(i)];
                const double* nj = &normal[3 * size_t(j)];
                const double dij = ni[0] * nj[0] + ni[1] * nj[1] + ni[2] * nj[2];
                if (dij < least) { least = dij; bi = i; bj = j; }
            }
        const double mid[3] = {normal[3 * size_t(bi)] + normal[3 * size_t(bj)], normal[3 * size_t(bi) + 1] + normal[3 * size_t(bj) + 1],
                               normal[3 * size_t(bi) + 2] + normal[3 * size_t(bj) + 2]};
        word = rf_cone_around(normal, lo, hi, mid);
    }
    return word;
}

// ---- normal slabs (the argument stands in rt_bvh.cpp) ----
// 1 / s of a node: s = 4 x its largest cell (cells are powers of two: exact), so that |x - org| / s <= 63.75 inside the node.
RT_HD inline double rf_slab_inv_scale(const float* cell) {
    const double cmax = rf_max(double(cell[0]), rf_max(double(cell[1]), double(cell[2])));
    return 0.25 / cmax;
}
// The margin of a slab in its own units: |q|_1 (2 pad / s + 2^-12), pad = rf_pad_of_box of the mesh.
RT_HD inline double rf_slab_margin(const int* q, double pad, double inv_s) {
    const double l1 = double((q[0] < 0 ? -q[0] : q[0]) + (q[1] < 0 ? -q[1] : q[1]) + (q[2] < 0 ? -q[2] : q[2]));
    return l1 * (2.0 * pad * inv_s + 1.0 / 4096.0);
}

// The three axis bytes of a cone word as integers.
RT_HD inline void rf_cone_axis(uint32_t cone, int* q) {
    q[0] = int(int8_t(cone & 0xFFu)); q[1] = int(int8_t((cone >> 8) & 0xFFu)); q[2] = int(int8_t((cone >> 16) & 0xFFu));
}
// Corner c (0: v0, 1: v0 + e1, 2: v0 + e2) of the record v = v0 e1 e2, as the slabs and the slab axes see it.
RT_HD inline void rf_tri_corner(const double* v, int c, double* x) {
    for (int a = 0; a < 3; a++) x[a] = c == 0 ? v[a] : v[a] + v[3 * c + a];
}
// P(x) = q . (x - org) / s of one corner, in this order of operations.
RT_HD inline double rf_slab_project(const int* q, const float* org, double inv_s, const double* x) {
    return double(q[0]) * ((x[0] - double(org[0])) * inv_s) + double(q[1]) * ((x[1] - double(org[1])) * inv_s) +
           double(q[2]) * ((x[2] - double(org[2])) * inv_s);
}
// The word of the exact interval [plo, phi] of P over the corners below a child: widened by rf_slab_margin, rounded outward.
RT_HD inline uint32_t rf_slab_finish(const int* q, double pad, double inv_s, double plo, double phi) {
    if (!(plo <= phi) || !std::isfinite(plo) || !std::isfinite(phi)) return kNeutralSlab;  // a NaN compares false
    const double margin = rf_slab_margin(q, pad, inv_s);
    const double l = rf_max(std::floor(plo - margin), -32768.0), h = rf_min(std::ceil(phi + margin), 32767.0);
    if (!(l <= 32767.0 && h >= -32768.0)) return kNeutralSlab;  // off the scale (a vertex outside the node's grid): no slab
    return (uint32_t(int32_t(l)) & 0xFFFFu) | (uint32_t(int32_t(h)) << 16);
}

// The slab word of a child with cone word `cone` over the slots [lo, hi), `count` triangles, in a node with grid origin
// `org` and cells `cell`: the exact interval of q . (x - org) / s over the three corners v0, v0 + e1, v0 + e2 of every
// triangle below, widened by rf_slab_margin and rounded outward to two signed 16-bit integers (lo | hi << 16).
// tri_at(slot, v) gives v0 e1 e2 in v[0..9).
template <typename TriAt>
RT_HD inline uint32_t rf_slab_word(uint32_t cone, const float* org, const float* cell, double pad, uint32_t lo, uint32_t hi, uint32_t count, TriAt tri_at) {
    if (cone == kNeutralCone || count == 0 || hi - lo != count) return kNeutralSlab;
    int q[3];
    rf_cone_axis(cone, q);
    const double inv_s = rf_slab_inv_scale(cell);
    if (!(inv_s > 0.0) || !std::isfinite(inv_s) || !std::isfinite(pad)) return kNeutralSlab;
    double plo = INFINITY, phi = -INFINITY;
    for (uint32_t t = lo; t < hi; t++) {
        double v[9];
        tri_at(t, v);
        for (int c = 0; c < 3; c++) {
            double x[3];
            rf_tri_corner(v, c, x);
            const double p = rf_slab_project(q, org, inv_s, x);
            plo = rf_min(plo, p);
            phi = rf_max(phi, p);
        }
    }
    return rf_slab_finish(q, pad, inv_s, plo, phi);
}

// ---- slab-only axes (the argument stands in rt_bvh.cpp) ----
// An inner child without a back-face cone (its normals go round too far) still profits from a slab if its surface is thin
// along SOME direction.  Such a child gets the cone word (qx, qy, qz, 127) with |q|_2 <= 126, which the cone test can never
// cull with, and the slab step reads q from it like any other axis.  q comes from a fixed table: the integer directions
// with components in -2..2 and at least two of them non-zero, one of every +- pair, reduced, each times the largest integer
// that keeps |q|_2 <= 126.  The six face diagonals stand first, then the four body diagonals: the first index wins ties.
// RT_SLAB_AXIS_COUNT (a prefix of the table: 10, 22 or 46) and RT_SLAB_AXIS_MAX_RATIO exist for the sweeps of
// profiles/slab_axes/README.md (tools/bvh_workmodel.cpp built with -D...); the library is built with the defaults.
#ifndef RT_SLAB_AXIS_COUNT
#define RT_SLAB_AXIS_COUNT 46
#endif
#ifndef RT_SLAB_AXIS_MAX_RATIO
#define RT_SLAB_AXIS_MAX_RATIO 0.9
#endif
constexpr int kSlabAxes = RT_SLAB_AXIS_COUNT;
static_assert(kSlabAxes >= 1 && kSlabAxes <= 46, "a prefix of the table");
constexpr double kSlabAxisMaxRatio = RT_SLAB_AXIS_MAX_RATIO;  // an axis is taken if the surface spans less than this share of its box along it
RT_HD inline void rf_slab_axis(int c, int* q) {
    static constexpr int8_t kTable[46][3] = {
        {0, 89, -89},   {0, 89, 89},    {89, -89, 0},   {89, 0, -89},    {89, 0, 89},    {89, 89, 0},    {72, -72, -72},  {72, -72, 72},
        {72, 72, -72},  {72, 72, 72},   {0, 56, -112},  {0, 56, 112},    {0, 112, -56},  {0, 112, 56},   {56, -112, 0},   {56, 0, -112},
        {56, 0, 112},   {56, 112, 0},   {112, -56, 0},  {112, 0, -56},   {112, 0, 56},   {112, 56, 0},   {42, -84, -84},  {51, -102, -51},
        {51, -102, 51}, {42, -84, 84},  {51, -51, -102}, {51, -51, 102}, {51, 51, -102}, {51, 51, 102},  {42, 84, -84},   {51, 102, -51},
        {51, 102, 51},  {42, 84, 84},   {84, -84, -42}, {84, -84, 42},   {84, -42, -84}, {102, -51, -51}, {102, -51, 51}, {84, -42, 84},
        {84, 42, -84},  {102, 51, -51}, {102, 51, 51},  {84, 42, 84},    {84, 84, -42},  {84, 84, 42}};
    q[0] = kTable[c][0]; q[1] = kTable[c][1]; q[2] = kTable[c][2];
}
// The support of a corner along a candidate: q . x in this order of operations.  Minima and maxima of it merge exactly.
RT_HD inline double rf_axis_project(const int* q, const double* x) { return double(q[0]) * x[0] + double(q[1]) * x[1] + double(q[2]) * x[2]; }

// May the child `ch` of a mesh with n_nodes 4-wide nodes (ch relative to the mesh's first node) get a slab-only axis?  An
// INNER child without a cone whose triangles are one run of slots [lo, hi), none of them ill-conditioned (`sum`, the sum of
// the normals below, is NaN otherwise).  Leaves keep their neutral words: a leaf without a cone is a fold or a coincident
// pair of a few triangles, and what a slab could save there is their tests, not a node visit.
RT_HD inline bool rf_slab_axis_eligible(int32_t ch, uint32_t n_nodes, uint32_t cone, uint32_t lo, uint32_t hi, uint32_t count, const double* sum) {
    if (ch < 0 || uint32_t(ch) >= n_nodes || cone != kNeutralCone) return false;  // kEmptyChild < 0
    if (count == 0 || hi - lo != count) return false;
    return std::isfinite(sum[0]) && std::isfinite(sum[1]) && std::isfinite(sum[2]);
}

// The candidate for a child with the exact box (blo, bhi), given smin / smax[c] = the exact min / max of rf_axis_project
// over the corners below: the one with the smallest (smax - smin) / sum_a |q_a| (bhi_a - blo_a), the first such, if that ratio
// is below kSlabAxisMaxRatio; else, or for a box that is flat or not finite, -1.
RT_HD inline int rf_slab_axis_pick(const double* blo, const double* bhi, const double* smin, const double* smax) {
    double ext[3];
    for (int a = 0; a < 3; a++) {
        ext[a] = bhi[a] - blo[a];
        if (!(ext[a] > 0.0) || !std::isfinite(ext[a])) return -1;
    }
    int best = -1;
    double best_ratio = kSlabAxisMaxRatio;
    for (int c = 0; c < kSlabAxes; c++) {
        int q[3];
        rf_slab_axis(c, q);
        const double den = double(q[0] < 0 ? -q[0] : q[0]) * ext[0] + double(q[1] < 0 ? -q[1] : q[1]) * ext[1] + double(q[2] < 0 ? -q[2] : q[2]) * ext[2];
        const double num = smax[c] - smin[c];
        if (!(num >= 0.0) || !std::isfinite(num) || !(den > 0.0) || !std::isfinite(den)) return -1;
        const double ratio = num / den;
        if (ratio < best_ratio) { best_ratio = ratio; best = c; }
    }
    return best;
}
// The slab-only cone word of candidate c.
RT_HD inline uint32_t rf_slab_axis_word(int c) {
    int q[3];
    rf_slab_axis(c, q);
    return uint32_t(q[0] & 0xFF) | (uint32_t(q[1] & 0xFF) << 8) | (uint32_t(q[2] & 0xFF) << 16) | (127u << 24);
}
// Is `cone` a slab-only word?  w = 127 and 0 < |q|_2 <= 126; the axis of a real cone is round(127 a) of a unit vector a, whose
// length is at least 127 - sqrt(3) / 2 > 126.
RT_HD inline bool rf_is_slab_only(uint32_t cone) {
    int q[3];
    rf_cone_axis(cone, q);
    const int l2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    return (cone >> 24) == 127u && l2 > 0 && l2 <= 126 * 126;
}

// RT_SLAB_AXES=0: no slab-only axes, the words of a child without a cone stay neutral (A/B control; read at every derivation).
bool slab_axes_enabled();

#if defined(__HIP__)
// ---- the device refit (rt_refit.hip) ----
// Everything one distinct mesh needs on the device to be refitted again and again: the leaf order, the index arrays and the
// relative child references of both trees (uploaded once, at the first update that moves the mesh), the vertex arrays of the
// last update and the scratch of the passes.  Shared by both arithmetic types.
struct RefitMesh {
    uint32_t n_tris = 0, n_nodes = 0, n_nodes4 = 0, n_positions = 0, n_normals = 0, n_uvs = 0;
    DevBuf<uint32_t> tri_order, tri_pos, tri_nrm;
    DevBuf<int32_t> tri_uv;             // NULL: the mesh has none
    DevBuf<int32_t> child2, child4;     // 2 / 4 per node; inner: node inside the mesh; leaf: ~(slot inside the mesh << 3 | count - 1)
    DevBuf<int32_t> parent2, parent4;   // -1: root
    DevBuf<uint32_t> inner2, inner4;    // inner children per node
    DevBuf<uint32_t> arrived2, arrived4;
    DevBuf<double> positions, normals, uvs;
    DevBuf<double> tri_box, tri_normal;  // per slot: lo xyz hi xyz / unit normal or NaN
    DevBuf<double> box2, box4;           // per node and child: lo xyz hi xyz (exact)
    DevBuf<double> sum4;                 // per node and child: sum of the normals below
    DevBuf<uint32_t> run4;               // per node and child: first slot, end slot, count
};

// Where the mesh's reader tables stand in the scene's device arrays of arithmetic type R.
template <typename R>
struct RefitTarget {
    BvhNode<R>* nodes;      // the mesh's first BVH2 node
    BvhNode4f* nodes4;      // its first 4-wide node
    MeshNode4qc* nodes4q;
    TriRec<R>* tris;        // its first record
    TriAttr<R>* attrs;
    double pad4;            // rf_pad_of_box of the mesh's new box
};

// Uploads the once-only arrays of the mesh (first call) and the vertex arrays of `m`.  *bytes += what went to the device.
bool refit_mesh_upload(RefitMesh& rm, const RtMesh& m, const uint32_t* tri_order, const int32_t* child2, uint32_t n_nodes, const int32_t* child4,
                       uint32_t n_nodes4, hipStream_t stream, uint64_t* bytes, std::string* err);
// The three passes for one arithmetic type, enqueued on `stream`.
template <typename R> bool refit_mesh_launch(RefitMesh& rm, const RefitTarget<R>& t, hipStream_t stream, std::string* err);
#endif  // __HIP__

}  // namespace rt
