// rt_traverse.h — the steps of a BVH search, each written ONCE: the clamped inverse direction, the exact triangle test, the
// two-child node step, the f32 culling ray, and the decode, cone cull and ordering of a 4-wide node's children, and the distance
// step of the point queries.  This is the only place that reads a BvhNode4q / MeshNode4qc header or a TriRec for intersection; a
// change of a node format starts here.
// Users: mesh_traverse (rt_device.h), k_wf_intersect, group_search and k_wf_mesh (rt_wavefront.h), mesh_any_hit (rt_query.h),
// mesh_closest (rt_point.h).
// The stacks and the loops around the steps stay with the kernels: they differ for measured reasons given there.
//
// Included by rt_device.h behind V3 / Lim / Ray, which everything here is written in.
#pragma once

namespace rt {

// Slab tests as t = b * inv - o * inv (culling only, any conservative test is admissible).
// A zero direction component gives inv = +-inf and inf - inf = NaN in that form, so the
// inverse used for them is clamped to a huge finite value: a ray parallel to a slab is then
// "inside forever" or "outside forever" - except ON one of the slab's planes: (plane - o) * inv is +-0 for that plane and
// -+huge for the other, so the slab comes out as (0, +huge) or as (-huge, 0), whichever the sign of the zero and the plane
// give.  On a padded box that is harmless (a ray on a padded plane is outside the true box); the tests that decide about a
// box with EXACT planes (span_misses, the scene program's mesh op) do not take an exit at exactly 0 for a miss.
template <typename R> RT_DEV V3<R> clamped_inv(const Ray<R>& ray) {
    const R big = sizeof(R) == 8 ? R(1e150) : R(1e18);
    return {fabs(ray.inv.x) > big ? copysign(big, ray.inv.x) : ray.inv.x,
            fabs(ray.inv.y) > big ? copysign(big, ray.inv.y) : ray.inv.y,
            fabs(ray.inv.z) > big ? copysign(big, ray.inv.z) : ray.inv.z};
}

// mesh.rs:62-107 Moeller-Trumbore with the reference's cull rule, up to the barycentric tests: true and (t, u, v) for a ray
// that crosses the triangle's plane inside it, outputs untouched otherwise.  The interval rule on t is the caller's.
// Callers hand in INITIALISED outputs: with undefined ones k_wf_intersect, the megakernel and the occlusion kernel came out
// 3-8 VGPRs larger than with the test written in place (profiles/traversal_steps/README.md).
template <typename R> RT_DEV bool tri_test(const TriRec<R>& tr, V3<R> o, V3<R> d, bool hit_back, R& t, R& u, R& v) {
    V3<R> edge1 = ld3(tr.e1), edge2 = ld3(tr.e2);
    V3<R> ray_x_edge2 = cross(d, edge2);
    R det = dot(edge1, ray_x_edge2);
    R dd = hit_back ? fabs(det) : det;
    if (!(dd < Lim<R>::det_eps())) {
        R inv_det = R(1) / det;
        V3<R> b = o - ld3(tr.v0);
        R uu = dot(b, ray_x_edge2) * inv_det;
        if (!(uu < R(0) || uu > R(1))) {
            V3<R> b_x_edge1 = cross(b, edge1);
            R vv = dot(d, b_x_edge1) * inv_det;
            if (!(vv < R(0) || uu + vv > R(1))) {
                t = dot(edge2, b_x_edge1) * inv_det;
                u = uu;
                v = vv;
                return true;
            }
        }
    }
    return false;
}

// BVH2 node (both children's boxes in the parent): true if the ray enters a child's box inside (t_lo, t_max); the one to
// visit next is `first`, and `second` the farther one if it enters both (kEmptyChild otherwise).  inv = clamped_inv(ray),
// oi = ray.o * inv.
template <typename R> RT_DEV bool node2_step(const BvhNode<R>& n, V3<R> inv, V3<R> oi, R t_lo, R t_max, int32_t& first, int32_t& second) {
    R t0x = n.lo0[0] * inv.x - oi.x, t1x = n.hi0[0] * inv.x - oi.x;
    R t0y = n.lo0[1] * inv.y - oi.y, t1y = n.hi0[1] * inv.y - oi.y;
    R t0z = n.lo0[2] * inv.z - oi.z, t1z = n.hi0[2] * inv.z - oi.z;
    R near0 = fmax(fmax(fmin(t0x, t1x), fmin(t0y, t1y)), fmax(fmin(t0z, t1z), t_lo));
    R far0 = fmin(fmin(fmax(t0x, t1x), fmax(t0y, t1y)), fmin(fmax(t0z, t1z), t_max));
    R s0x = n.lo1[0] * inv.x - oi.x, s1x = n.hi1[0] * inv.x - oi.x;
    R s0y = n.lo1[1] * inv.y - oi.y, s1y = n.hi1[1] * inv.y - oi.y;
    R s0z = n.lo1[2] * inv.z - oi.z, s1z = n.hi1[2] * inv.z - oi.z;
    R near1 = fmax(fmax(fmin(s0x, s1x), fmin(s0y, s1y)), fmax(fmin(s0z, s1z), t_lo));
    R far1 = fmin(fmin(fmax(s0x, s1x), fmax(s0y, s1y)), fmin(fmax(s0z, s1z), t_max));
    int32_t c0 = n.c0, c1 = n.c1;
    bool h0 = (near0 <= far0) && c0 != kEmptyChild;
    bool h1 = (near1 <= far1) && c1 != kEmptyChild;
    second = kEmptyChild;
    if (h0 && h1) {
        bool first0 = near0 <= near1;
        second = first0 ? c1 : c0;
        first = first0 ? c0 : c1;
        return true;
    }
    if (h0) { first = c0; return true; }
    if (h1) { first = c1; return true; }
    return false;
}

// f32 value that is certainly >= x (x finite or +inf): round to nearest, then add a relative margin.
template <typename R> RT_DEV float f32_at_least(R x) {
    float f = float(x);
    return f + fabsf(f) * 9.5367431640625e-7f + 1e-30f;  // 2^-20 relative
}

// The f32 culling ray of the 4-wide nodes: the exact ray with its origin moved to o + d * t_shift, where it enters the box
// that holds the tree, so that |origin| is no larger than the box (the nodes' padding covers the slab test's rounding for
// such origins, rt_scene.h BvhNode4f); t is measured from there.  The near plane of an axis follows from the sign of iv.
template <typename R>
struct CullRay {
    float ivx, ivy, ivz;  // 1 / d, clamped like clamped_inv
    float oix, oiy, oiz;  // moved origin * iv
    R t_shift;
    RT_DEV bool negx() const { return ivx < 0.0f; }
    RT_DEV bool negy() const { return ivy < 0.0f; }
    RT_DEV bool negz() const { return ivz < 0.0f; }
};
// Builds it from the exact ray and the box [lo, hi]; t_shift is the entry into the box, at least `floor`.  t_enter (t_shift
// before its guard) and t_exit are what the caller's miss rule needs.
template <typename R> RT_DEV CullRay<R> make_cull_ray(const Ray<R>& ray, const R* lo, const R* hi, R floor, R& t_enter, R& t_exit) {
    const V3<R> inv = clamped_inv(ray);
    const R e0x = (lo[0] - ray.o.x) * inv.x, e1x = (hi[0] - ray.o.x) * inv.x;
    const R e0y = (lo[1] - ray.o.y) * inv.y, e1y = (hi[1] - ray.o.y) * inv.y;
    const R e0z = (lo[2] - ray.o.z) * inv.z, e1z = (hi[2] - ray.o.z) * inv.z;
    t_enter = fmax(fmax(fmin(e0x, e1x), fmin(e0y, e1y)), fmax(fmin(e0z, e1z), floor));
    t_exit = fmin(fmin(fmax(e0x, e1x), fmax(e0y, e1y)), fmax(e0z, e1z));
    CullRay<R> cr;
    cr.t_shift = fabs(t_enter) < Lim<R>::inf() ? t_enter : R(0);
    const V3<R> oc = ray.o + ray.d * cr.t_shift;
    const float big32 = 1e18f;
    cr.ivx = 1.0f / float(ray.d.x); cr.ivy = 1.0f / float(ray.d.y); cr.ivz = 1.0f / float(ray.d.z);
    cr.ivx = fabsf(cr.ivx) > big32 ? copysignf(big32, cr.ivx) : cr.ivx;
    cr.ivy = fabsf(cr.ivy) > big32 ? copysignf(big32, cr.ivy) : cr.ivy;
    cr.ivz = fabsf(cr.ivz) > big32 ? copysignf(big32, cr.ivz) : cr.ivz;
    cr.oix = float(oc.x) * cr.ivx; cr.oiy = float(oc.y) * cr.ivy; cr.oiz = float(oc.z) * cr.ivz;
    return cr;
}
// The miss rule of the callers that have one: the ray leaves the box before it enters it, or enters it behind t_max - a miss
// only if it is one with a few ulps of slack on both ends (a NaN compares false: the tree is searched).
// An exit at exactly 0 is no miss either: the origin lies ON a plane of the box, and if the ray runs parallel to that plane
// (clamped_inv) it stays on the closed box and hits what lies there - the border of a grid straight down, a face of a cube
// along it, the outermost sphere of a group on a tangent.  Half of those rays came out as (-huge, 0) and were dropped.  The
// other rays with that exit leave the box where they start; searching the tree for them costs a visit of the root.
template <typename R> RT_DEV bool span_misses(R t_enter, R t_exit, R t_max) {
    const R eps = Lim<R>::eps() * R(16);
    return (t_enter - fabs(t_enter) * eps > t_exit + fabs(t_exit) * eps && t_exit != R(0)) || (t_enter - fabs(t_enter) * eps > t_max);
}

// Object-space direction as four signed bytes (round(127 d / |d|), -127) for the back-face cone test (rt_bvh.cpp has the
// argument); kNoCullDir, the word that culls nothing, if culling is not allowed (switched off, or a mesh that hits back
// faces) or |d|^2 is outside the range (or NaN: a non-finite component).
template <typename R> RT_DEV uint32_t quantise_dir(V3<R> d, bool cull_allowed) {
    const R len2 = d.x * d.x + d.y * d.y + d.z * d.z;
    const R len_lo = sizeof(R) == 8 ? R(1e-200) : R(1e-24), len_hi = sizeof(R) == 8 ? R(1e200) : R(1e24);
    uint32_t dirq = kNoCullDir;
    if (cull_allowed && len2 > len_lo && len2 < len_hi) {
        const R sc127 = R(127) / sqrt(len2);
        const int qx = int(rint(d.x * sc127)), qy = int(rint(d.y * sc127)), qz = int(rint(d.z * sc127));
        dirq = (uint32_t(qx) & 0xFFu) | ((uint32_t(qy) & 0xFFu) << 8) | ((uint32_t(qz) & 0xFFu) << 16) | kNoCullDir;
    }
    return dirq;
}

// Children of a MeshNode4qc (cn: its fifth 16 bytes, cc: its child references): a child whose triangles all face away from
// the ray (dir . cone > 0) counts as empty.
RT_DEV void node4q_cull_cones(uint32_t dirq, uint4 cn, int4 cc, int32_t (&ch)[4]) {
    ch[0] = __builtin_amdgcn_sdot4(int(dirq), int(cn.x), 0, false) > 0 ? kEmptyChild : cc.x;
    ch[1] = __builtin_amdgcn_sdot4(int(dirq), int(cn.y), 0, false) > 0 ? kEmptyChild : cc.y;
    ch[2] = __builtin_amdgcn_sdot4(int(dirq), int(cn.z), 0, false) > 0 ? kEmptyChild : cc.z;
    ch[3] = __builtin_amdgcn_sdot4(int(dirq), int(cn.w), 0, false) > 0 ? kEmptyChild : cc.w;
}

constexpr float kNoEntry = __builtin_huge_valf();  // entry distance of a child that is not entered

// Slab test of the four child boxes of a BvhNode4q (h0..h2: its first 48 bytes) against the culling ray up to tmax32:
// nr[k] = entry distance of child k, kNoEntry if the ray misses its box or ch[k] is kEmptyChild; bit k of the result says which.
// plane = org + q * cell, so t = q * (cell * iv) + (org * iv - o * iv).  Explicit FMAs: the translation unit is built with
// -ffp-contract=off for the f64 parity arithmetic, but this f32 test only culls (its rounding is inside the boxes' padding
// either way).
// fr[k] = the exit distance of child k (what the entry was compared with), for node4q_cull_slabs.
template <typename R>
RT_DEV uint32_t node4q_spans(uint4 h0, uint4 h1, uint4 h2, const CullRay<R>& cr, float tmax32, const int32_t (&ch)[4], float (&nr)[4], float (&fr)[4]) {
    const float ax = __uint_as_float(h0.w) * cr.ivx, ay = __uint_as_float(h1.x) * cr.ivy, az = __uint_as_float(h1.y) * cr.ivz;
    const float bx = fmaf(__uint_as_float(h0.x), cr.ivx, -cr.oix), by = fmaf(__uint_as_float(h0.y), cr.ivy, -cr.oiy), bz = fmaf(__uint_as_float(h0.z), cr.ivz, -cr.oiz);
    // with lo <= hi the nearer plane of an axis is `lo` for a non-negative inverse direction, `hi` otherwise:
    // lo * iv vs hi * iv are then already ordered and the per-box min/max disappear
    const bool negx = cr.negx(), negy = cr.negy(), negz = cr.negz();
    const uint32_t qnx = negx ? h2.y : h1.z, qfx = negx ? h1.z : h2.y;
    const uint32_t qny = negy ? h2.z : h1.w, qfy = negy ? h1.w : h2.z;
    const uint32_t qnz = negz ? h2.w : h2.x, qfz = negz ? h2.x : h2.w;
    uint32_t entered = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float nxk = float((qnx >> (8 * k)) & 0xFFu), nyk = float((qny >> (8 * k)) & 0xFFu), nzk = float((qnz >> (8 * k)) & 0xFFu);
        const float fxk = float((qfx >> (8 * k)) & 0xFFu), fyk = float((qfy >> (8 * k)) & 0xFFu), fzk = float((qfz >> (8 * k)) & 0xFFu);
        const float tn = fmaxf(fmaxf(fmaf(nxk, ax, bx), fmaf(nyk, ay, by)), fmaxf(fmaf(nzk, az, bz), 0.0f));
        const float tf = fminf(fminf(fmaf(fxk, ax, bx), fmaf(fyk, ay, by)), fminf(fmaf(fzk, az, bz), tmax32));
        const bool h = (tn <= tf) && ch[k] != kEmptyChild;
        nr[k] = h ? tn : kNoEntry;
        fr[k] = tf;
        entered |= uint32_t(h) << k;
    }
    return entered;
}
template <typename R>
RT_DEV uint32_t node4q_entries(uint4 h0, uint4 h1, uint4 h2, const CullRay<R>& cr, float tmax32, const int32_t (&ch)[4], float (&nr)[4]) {
    float fr[4];
    return node4q_spans(h0, h1, h2, cr, tmax32, ch, nr, fr);
}

// Normal slabs of a MeshNode4qc (cn: its cone words, sl: its sixth 16 bytes; builder and proof: rt_bvh.cpp): an entered child
// whose span [nr, fr] of the culling ray lies wholly below or wholly above its slab becomes "not entered".  (o, d, t_shift):
// the exact ray and where the culling ray starts on it.  leaves_only: RT_WF_SLABS=2.  nr[] of the children that stay, their
// order and everything behind this step are untouched.  Explicit FMAs, as in node4q_spans.  The axis is whatever the three axis
// bytes of the cone word say: a back-face cone's, or the slab-only axis of a child without a cone (w = 127, never culls as a
// cone); only kNeutralCone has q = 0 and with it no slab.
template <typename R>
RT_DEV void node4q_cull_slabs(uint4 h0, uint4 h1, uint4 cn, uint4 sl, V3<R> o, V3<R> d, R t_shift, bool leaves_only, const int32_t (&ch)[4],
                              const float (&fr)[4], float (&nr)[4]) {
    const float cmax = fmaxf(fmaxf(__uint_as_float(h0.w), __uint_as_float(h1.x)), __uint_as_float(h1.y));
    const float inv_s = __uint_as_float(0x7E000000u - __float_as_uint(cmax));  // 1 / (4 cmax): cmax = 2^e, e in [-100, 120]
    const float rx = (float(fma(d.x, t_shift, o.x)) - __uint_as_float(h0.x)) * inv_s;
    const float ry = (float(fma(d.y, t_shift, o.y)) - __uint_as_float(h0.y)) * inv_s;
    const float rz = (float(fma(d.z, t_shift, o.z)) - __uint_as_float(h0.z)) * inv_s;
    float ex = float(d.x) * inv_s;
    const float ey = float(d.y) * inv_s, ez = float(d.z) * inv_s;
    // the range the proof covers: direction 1e-20 < max |e| < 1e30, node no farther than 2^16 s from the origin and from the ray's
    // start.  Outside it every pn, pf is NaN and nothing is culled.
    const float em = fmaxf(fmaxf(fabsf(ex), fabsf(ey)), fabsf(ez));
    const float gm = fmaxf(fmaxf(fmaxf(fabsf(__uint_as_float(h0.x)), fabsf(__uint_as_float(h0.y))), fabsf(__uint_as_float(h0.z))) * inv_s,
                           fmaxf(fmaxf(fabsf(rx), fabsf(ry)), fabsf(rz)));
    if (!(em > 1e-20f && em < 1e30f && gm < 65536.0f)) ex = __builtin_nanf("");
    const uint32_t cw[4] = {cn.x, cn.y, cn.z, cn.w}, sw[4] = {sl.x, sl.y, sl.z, sl.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float qx = float(int(cw[k] << 24) >> 24), qy = float(int(cw[k] << 16) >> 24), qz = float(int(cw[k] << 8) >> 24);
        const float A = fmaf(qx, rx, fmaf(qy, ry, qz * rz));
        const float B = fmaf(qx, ex, fmaf(qy, ey, qz * ez));
        const float pn = fmaf(nr[k], B, A), pf = fmaf(fr[k], B, A);
        const float lo = float(int(sw[k] << 16) >> 16), hi = float(int(sw[k]) >> 16);
        // both ends below lo or both above hi, without branches: fmaxf / fminf drop a NaN operand, and the only way to ONE NaN
        // is tf = +inf with B = 0, where the true pf equals pn; with both NaN the comparisons fail
        const bool out = bool(int(fmaxf(pn, pf) < lo) | int(fminf(pn, pf) > hi));
        const bool may = bool(int(!leaves_only) | int(ch[k] < 0));
        nr[k] = bool(int(out) & int(may)) ? kNoEntry : nr[k];
    }
}

// Lower bound on the squared distance from the point q to the box [lo, hi], all three in R, whatever roundings produced them:
// per axis the gap max(lo - q, q - hi, 0) is taken in R and then shrunk by 2 eps (|q| + max(|lo|, |hi|)), eps = Lim<R>::eps()
// = two unit roundoffs, which covers a rounding of q (the f64 point rounded to R, one unit roundoff of |q|), a rounding of
// the plane (one of |plane|) and the subtraction's own (one of the gap, itself at most |q| + |plane|) with a unit roundoff
// of each to spare; the sum of the three squares is shrunk by 4 eps for its five roundings.  Nothing here leans on the
// boxes' padding (DESIGN.md section 20 has the argument in full).  A NaN anywhere gives NaN: the caller's `lb < r2` is false.
template <typename R> RT_DEV R box_dist2_below(V3<R> lo, V3<R> hi, V3<R> q) {
    const R e2 = Lim<R>::eps() * R(2);
    const R gx = fmax(fmax(lo.x - q.x, q.x - hi.x), R(0)) - e2 * (fabs(q.x) + fmax(fabs(lo.x), fabs(hi.x)));
    const R gy = fmax(fmax(lo.y - q.y, q.y - hi.y), R(0)) - e2 * (fabs(q.y) + fmax(fabs(lo.y), fabs(hi.y)));
    const R gz = fmax(fmax(lo.z - q.z, q.z - hi.z), R(0)) - e2 * (fabs(q.z) + fmax(fabs(lo.z), fabs(hi.z)));
    const R ax = gx > R(0) ? gx : R(0), ay = gy > R(0) ? gy : R(0), az = gz > R(0) ? gz : R(0);
    return (ax * ax + ay * ay + az * az) * (R(1) - Lim<R>::eps() * R(4));
}

// Distance step of a point query over a BvhNode4q (h0..h2: its first 48 bytes): lb[k] = a lower bound on the squared
// object-space distance from q to child k's decoded box (box_dist2_below on planes decoded in R: org + q * cell, the product
// exact, the sum rounded once in f32 and exact or rounded once in f64), kNoEntry for ch[k] == kEmptyChild.  No cone or slab
// word is read: facing does not matter to a distance.
template <typename R> RT_DEV void node4q_dist2(uint4 h0, uint4 h1, uint4 h2, V3<R> q, const int32_t (&ch)[4], R (&lb)[4]) {
    const R ox = R(__uint_as_float(h0.x)), oy = R(__uint_as_float(h0.y)), oz = R(__uint_as_float(h0.z));
    const R cx = R(__uint_as_float(h0.w)), cy = R(__uint_as_float(h1.x)), cz = R(__uint_as_float(h1.y));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const V3<R> lo = {ox + R((h1.z >> (8 * k)) & 0xFFu) * cx, oy + R((h1.w >> (8 * k)) & 0xFFu) * cy, oz + R((h2.x >> (8 * k)) & 0xFFu) * cz};
        const V3<R> hi = {ox + R((h2.y >> (8 * k)) & 0xFFu) * cx, oy + R((h2.z >> (8 * k)) & 0xFFu) * cy, oz + R((h2.w >> (8 * k)) & 0xFFu) * cz};
        lb[k] = ch[k] != kEmptyChild ? box_dist2_below(lo, hi, q) : R(kNoEntry);
    }
}

// f32 value that is certainly <= x for x >= 0 (finite or +inf; +inf and values beyond the f32 range give FLT_MAX).
template <typename R> RT_DEV float f32_at_most(R x) {
    const float f = fminf(float(x), 3.402823466e+38f);
    return f < 1e-30f ? 0.0f : f - f * 9.5367431640625e-7f;  // 2^-20 relative; below the range where that is 8 ulps: 0
}

// Sorts the four (entry distance, child) pairs of the arrays nr / ch in place, nearest first (5 compare-exchanges); kNoEntry
// children end up last.  The one step that is a macro: as a function on references to the arrays it cost k_wf_prims<GROUPS>
// two VGPRs in f64 (127 -> 129), on copies of them one in f32 (96 -> 97), each across an allocation boundary
// (profiles/traversal_steps/README.md).
#define RT_CE(nr, ch, a, b)                                           \
    if (nr[a] > nr[b]) {                                              \
        float tn_ = nr[a]; nr[a] = nr[b]; nr[b] = tn_;                \
        int32_t tc_ = ch[a]; ch[a] = ch[b]; ch[b] = tc_;              \
    }
#define RT_SORT4_NEAREST_FIRST(nr, ch) RT_CE(nr, ch, 0, 1) RT_CE(nr, ch, 2, 3) RT_CE(nr, ch, 0, 2) RT_CE(nr, ch, 1, 3) RT_CE(nr, ch, 1, 2)

}  // namespace rt
