// Binned-SAH BVH2 builder (host, f64).  See rt_bvh.h.
#include "rt_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "rt_refit.h"
#include "rt_scene.h"

namespace rt {
namespace {

constexpr int kMaxBins = 64;
static int g_bins = 16;  // RT_BVH_BINS (experiments)
constexpr double kInf = std::numeric_limits<double>::infinity();

struct Box {
    double lo[3] = {kInf, kInf, kInf};
    double hi[3] = {-kInf, -kInf, -kInf};
    void grow(const double* p) {
        for (int a = 0; a < 3; a++) {
            if (p[a] < lo[a]) lo[a] = p[a];
            if (p[a] > hi[a]) hi[a] = p[a];
        }
    }
    void grow(const Box& b) {
        for (int a = 0; a < 3; a++) {
            if (b.lo[a] < lo[a]) lo[a] = b.lo[a];
            if (b.hi[a] > hi[a]) hi[a] = b.hi[a];
        }
    }
    double half_area() const {
        double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.0;
        return dx * dy + dy * dz + dz * dx;
    }
};

struct Builder {
    std::vector<Box> tri_box;
    std::vector<double> centroid;  // n*3
    std::vector<uint32_t> order;
    std::vector<BuildNode> nodes;
    uint32_t max_leaf;
    uint32_t max_depth = 0;

    static int32_t leaf_ref(uint32_t first, uint32_t count) { return ~int32_t((first << 3) | (count - 1)); }

    // Builds the subtree over order[begin, end); returns the child reference and its box.
    int32_t build(uint32_t begin, uint32_t end, Box* out_box, uint32_t depth) {
        Box box, cbox;
        for (uint32_t i = begin; i < end; i++) {
            box.grow(tri_box[order[i]]);
            cbox.grow(&centroid[3 * order[i]]);
        }
        *out_box = box;
        uint32_t n = end - begin;
        if (n <= max_leaf) return leaf_ref(begin, n);

        // pick axis/plane by binned SAH over centroid bounds
        int best_axis = -1, best_bin = -1;
        double best_cost = kInf;
        for (int a = 0; a < 3; a++) {
            double ext = cbox.hi[a] - cbox.lo[a];
            if (!(ext > 0.0) || !std::isfinite(ext)) continue;
            const int kBins = g_bins;
            Box bins[kMaxBins];
            uint32_t counts[kMaxBins] = {0};
            double scale = double(kBins) / ext;
            for (uint32_t i = begin; i < end; i++) {
                int b = int((centroid[3 * order[i] + a] - cbox.lo[a]) * scale);
                if (b < 0) b = 0;
                if (b >= kBins) b = kBins - 1;
                bins[b].grow(tri_box[order[i]]);
                counts[b]++;
            }
            double right_area[kMaxBins];
            uint32_t right_count[kMaxBins];
            Box acc;
            uint32_t cnt = 0;
            for (int b = kBins - 1; b > 0; b--) {
                acc.grow(bins[b]);
                cnt += counts[b];
                right_area[b] = acc.half_area();
                right_count[b] = cnt;
            }
            Box lacc;
            uint32_t lcnt = 0;
            for (int b = 0; b < kBins - 1; b++) {
                lacc.grow(bins[b]);
                lcnt += counts[b];
                if (lcnt == 0 || right_count[b + 1] == 0) continue;
                double cost = lacc.half_area() * double(lcnt) + right_area[b + 1] * double(right_count[b + 1]);
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = a;
                    best_bin = b;
                }
            }
        }
        uint32_t mid;
        if (best_axis < 0) {
            mid = begin + n / 2;  // all centroids coincide (or non-finite): split by index
        } else {
            const int kBins = g_bins;
            double ext = cbox.hi[best_axis] - cbox.lo[best_axis];
            double scale = double(kBins) / ext;
            double lo = cbox.lo[best_axis];
            auto it = std::partition(order.begin() + begin, order.begin() + end, [&](uint32_t t) {
                int b = int((centroid[3 * t + best_axis] - lo) * scale);
                if (b < 0) b = 0;
                if (b >= kBins) b = kBins - 1;
                return b <= best_bin;
            });
            mid = uint32_t(it - order.begin());
            if (mid == begin || mid == end) mid = begin + n / 2;
        }
        uint32_t idx = uint32_t(nodes.size());
        nodes.emplace_back();
        if (depth + 1 > max_depth) max_depth = depth + 1;
        Box b0, b1;
        int32_t c0 = build(begin, mid, &b0, depth + 1);
        int32_t c1 = build(mid, end, &b1, depth + 1);
        BuildNode& nd = nodes[idx];
        for (int a = 0; a < 3; a++) {
            nd.lo0[a] = b0.lo[a]; nd.hi0[a] = b0.hi[a];
            nd.lo1[a] = b1.lo[a]; nd.hi1[a] = b1.hi[a];
        }
        nd.c0 = c0;
        nd.c1 = c1;
        return int32_t(idx);
    }
};

}  // namespace

BvhBuild build_bvh(const double* positions, const uint32_t* tri_pos, uint32_t n_tris, uint32_t max_leaf) {
    if (const char* e = std::getenv("RT_BVH_BINS")) { int v = std::atoi(e); if (v >= 2 && v <= kMaxBins) g_bins = v; }
    Builder b;
    b.max_leaf = std::min<uint32_t>(std::max<uint32_t>(max_leaf, 1), 8);
    b.tri_box.resize(n_tris);
    b.centroid.resize(size_t(n_tris) * 3);
    b.order.resize(n_tris);
    for (uint32_t t = 0; t < n_tris; t++) {
        b.order[t] = t;
        Box bx;
        for (int k = 0; k < 3; k++) bx.grow(positions + 3 * size_t(tri_pos[3 * size_t(t) + k]));
        b.tri_box[t] = bx;
        for (int a = 0; a < 3; a++) b.centroid[3 * size_t(t) + a] = 0.5 * (bx.lo[a] + bx.hi[a]);
    }
    b.nodes.reserve(n_tris / 2 + 4);
    BvhBuild out;
    if (n_tris <= b.max_leaf) {
        // Tiny mesh: a root whose first child is the only leaf.
        BuildNode root{};
        Box bx;
        for (uint32_t t = 0; t < n_tris; t++) bx.grow(b.tri_box[t]);
        for (int a = 0; a < 3; a++) {
            root.lo0[a] = bx.lo[a]; root.hi0[a] = bx.hi[a];
            root.lo1[a] = kInf; root.hi1[a] = -kInf;
        }
        root.c0 = n_tris ? Builder::leaf_ref(0, n_tris) : kEmptyChild;
        root.c1 = kEmptyChild;
        out.nodes.push_back(root);
        out.max_depth = 1;
    } else {
        Box root_box;
        b.build(0, n_tris, &root_box, 0);  // n > max_leaf: the root is an inner node at index 0
        out.nodes = std::move(b.nodes);
        out.max_depth = b.max_depth;
    }
    out.tri_order = std::move(b.order);
    return out;
}


namespace {
struct Cand {
    int32_t ref;
    double lo[3], hi[3];
    double area() const {
        double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (!(dx >= 0 && dy >= 0 && dz >= 0)) return -1.0;
        return dx * dy + dy * dz + dz * dx;
    }
};
template <int W>
struct Collapser {
    const BvhBuild& b2;
    BvhNBuild<W> out;
    uint32_t build(int32_t n2, uint32_t depth, uint32_t stack_above) {
        uint32_t idx = uint32_t(out.nodes.size());
        out.nodes.emplace_back();
        if (depth + 1 > out.max_depth) out.max_depth = depth + 1;
        std::vector<Cand> c;
        auto add_children = [&](int32_t node2) {
            const BuildNode& n = b2.nodes[size_t(node2)];
            Cand a{n.c0, {n.lo0[0], n.lo0[1], n.lo0[2]}, {n.hi0[0], n.hi0[1], n.hi0[2]}};
            Cand b{n.c1, {n.lo1[0], n.lo1[1], n.lo1[2]}, {n.hi1[0], n.hi1[1], n.hi1[2]}};
            if (a.ref != kEmptyChild) c.push_back(a);
            if (b.ref != kEmptyChild) c.push_back(b);
        };
        add_children(n2);
        for (;;) {
            if (c.size() >= size_t(W)) break;
            int best = -1;
            double best_area = -1.0;
            for (size_t i = 0; i < c.size(); i++)
                if (c[i].ref >= 0 && c[i].area() > best_area) { best_area = c[i].area(); best = int(i); }
            if (best < 0) break;  // only leaves left
            int32_t expand = c[size_t(best)].ref;
            c.erase(c.begin() + best);
            add_children(expand);
        }
        uint32_t n_children = uint32_t(c.size());
        uint32_t stack_here = stack_above + (n_children > 0 ? n_children - 1 : 0);
        if (stack_here + 1 > out.max_stack) out.max_stack = stack_here + 1;
        BuildNodeN<W> node{};
        for (int k = 0; k < W; k++) {
            node.child[k] = kEmptyChild;
            for (int a = 0; a < 3; a++) { node.lo[k][a] = kInf; node.hi[k][a] = -kInf; }
        }
        for (uint32_t k = 0; k < n_children; k++) {
            for (int a = 0; a < 3; a++) { node.lo[k][a] = c[k].lo[a]; node.hi[k][a] = c[k].hi[a]; }
            node.child[k] = c[k].ref;  // inner refs are patched below
        }
        out.nodes[idx] = node;
        for (uint32_t k = 0; k < n_children; k++)
            if (c[k].ref >= 0) {
                uint32_t child_idx = build(c[k].ref, depth + 1, stack_here);
                out.nodes[idx].child[k] = int32_t(child_idx);
            }
        return idx;
    }
};
}  // namespace

namespace {
template <int W>
BvhNBuild<W> collapse(const BvhBuild& b2) {
    Collapser<W> c{b2, {}};
    c.out.nodes.reserve(b2.nodes.size() / (W == 4 ? 2 : 3) + 4);
    c.build(0, 0, 0);
    for (int a = 0; a < 3; a++) { c.out.root_lo[a] = kInf; c.out.root_hi[a] = -kInf; }
    const BuildNodeN<W>& r = c.out.nodes[0];
    for (int k = 0; k < W; k++)
        if (r.child[k] != kEmptyChild)
            for (int a = 0; a < 3; a++) {
                c.out.root_lo[a] = std::min(c.out.root_lo[a], r.lo[k][a]);
                c.out.root_hi[a] = std::max(c.out.root_hi[a], r.hi[k][a]);
            }
    return std::move(c.out);
}
}  // namespace

Bvh4Build collapse_bvh4(const BvhBuild& b2) { return collapse<4>(b2); }


// ---------------------------------------------------------------------------------------------
// Back-face cones of the 4-wide mesh nodes.
//
// The triangle test of k_wf_mesh (the reference's, mesh.rs:62-107) computes det = e1 . (d x e2) = -d . (e1 x e2) and
// rejects the triangle if det < EPSILON, unless the mesh hits back faces.  A child all of whose triangles face away from
// the ray can therefore be skipped without changing the closest hit, the order of the remaining tests included.
//
// Per child: n_i = unit normals e1 x e2 of the triangles below it, a = q / |q| with q = round(127 x their normalised sum)
// (the axis as the kernel sees it; for a leaf whose sum gives no cone, the bisector of its two normals farthest apart),
// c = min_i a . n_i (the exact minimum over the triangles, not a merge of child cones), s = sqrt(1 - c^2),
// w = ceil(|q| (s + d_dir + d_safe)); the word is (q, w), valid if c >= kConeMinCos and w <= 127.
// The kernel packs D = (round(127 d / |d|), -127) and culls the child if D . (q, w) > 0 in integer arithmetic.
//
//  1. Every byte of D is within 0.5 + 1e-4 of 127 d^ (d^ = d / |d|; the 1e-4 covers normalising in f32), so
//     127 d^ . q >= D_xyz . q - (sqrt(3) / 2 + 2e-4) |q| > 127 w - 127 d_dir |q| >= 127 |q| (s + d_safe), with
//     d_dir = 0.00682 >= (sqrt(3) / 2 + 2e-4) / 127: cos(theta) = d^ . a > s + d_safe.
//  2. Every n_i is within alpha = acos(c) of a, so d^ . n_i >= cos(theta + alpha) = cos(theta) c - sin(theta) s
//     >= (s + d_safe) c - c s = d_safe c  (sin(theta) <= sqrt(1 - s^2) = c).  The host's own rounding in a, n_i and c is
//     below 1e-14 and is charged to d_safe: 0.9 d_safe is what the next step uses.
//  3. det_true = -|d| |e1 x e2| d^ . n_i <= -0.9 d_safe c sigma |d| |e1| |e2| for a well-conditioned triangle
//     (|e1 x e2| >= sigma |e1| |e2|).
//  4. The computed det: each component of d x e2 is fl(fl(ab) - fl(cd)), off by at most 3u (|ab| + |cd|) <= 3u |d| |e2|
//     per component, 3 sqrt(3) u |d| |e2| as a vector; the three-term dot adds 3u |e1| |d x e2|; no contraction
//     (-ffp-contract=off).  Together |det - det_true| <= gamma |d| |e1| |e2| with gamma = 10u (u = 2^-53: 1.1e-15).
//     In f32 builds the records are the f64 edges rounded to f32, which moves e1 x e2 by at most 2u |e1| |e2|:
//     gamma = 12u (u = 2^-24: 7.2e-7).
//  5. With 0.9 d_safe c sigma > gamma the computed det is negative, `det < EPSILON` holds and the test returns "no hit".
//     d_safe = 1e-3, c >= 1/8: f64, sigma = 2^-20: 1.07e-10 > 1.1e-15 (five orders to spare);
//     f32, sigma = 2^-5: 3.5e-6 > 7.2e-7.
//  6. Under- and overflow: edges outside [min_edge, max_edge] make a triangle ill-conditioned, and the kernel gives the
//     never-culling direction word to rays with |d|^2 outside [1e-24, 1e24] (f32) / [1e-200, 1e200] (f64), so no product of
//     step 4 overflows; an underflow moves det by less than the smallest normal number, far inside EPSILON.
//     Non-finite directions and coordinates are excluded the same way: a NaN det PASSES `!(det < EPSILON)`.
//     Meshes that hit back faces test |det|; the kernel never culls for them.
//
// A child above an ill-conditioned triangle, an empty child, a child whose cone is wider than acos(kConeMinCos) and (never seen:
// both builders order the triangles subtree by subtree) a child whose triangles are not one run of slots get kNeutralCone.
// ---------------------------------------------------------------------------------------------
// d_dir, d_safe and the bound on c (kConeDirSlack, kConeSafety, kConeMinCos) and the per-child formulas stand in rt_refit.h:
// the refit kernels of rt_scene_update evaluate the same functions on the device.

ConeLimits cone_limits(bool f32) {
    if (f32) return ConeLimits{1.0 / 32.0, 1e-12, 1e12};
    return ConeLimits{1.0 / 1048576.0, 1e-100, 1e100};
}

void build_mesh_cones(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const ConeLimits& lim,
                      std::vector<uint32_t>* out) {
    const size_t n_tris = tris.size();
    // unit normals; a triangle that is ill-conditioned has normal[3 t] = NaN
    std::vector<double> normal(3 * n_tris);
    const double kNaN = std::numeric_limits<double>::quiet_NaN();
    for (size_t t = 0; t < n_tris; t++) rf_tri_normal(tris[t].v0, tris[t].e1, tris[t].e2, lim, &normal[3 * t]);
    // what lies below a child: the run of triangle slots [lo, hi), their number, the sum of their normals (NaN if one is bad)
    struct Below {
        uint32_t lo = UINT32_MAX, hi = 0, count = 0;
        double sum[3] = {0.0, 0.0, 0.0};
        void add(const Below& o) {
            lo = std::min(lo, o.lo); hi = std::max(hi, o.hi); count += o.count;
            for (int a = 0; a < 3; a++) sum[a] += o.sum[a];
        }
    };
    auto cone_word = [&](const Below& b) -> uint32_t { return rf_cone_word(normal.data(), b.lo, b.hi, b.count, b.sum); };
    out->assign(4 * nodes4.size(), kNeutralCone);
    std::vector<Below> below(nodes4.size());  // per node: the union of its children
    for (size_t i = nodes4.size(); i-- > 0;) {  // children stand behind their parent: bottom-up without recursion
        const BuildNode4& nd = nodes4[i];
        Below all;
        for (int k = 0; k < 4; k++) {
            const int32_t ch = nd.child[k];
            if (ch == kEmptyChild) continue;
            Below b;
            if (ch >= 0) {
                if (size_t(ch) <= i || size_t(ch) >= nodes4.size()) { all.sum[0] = kNaN; continue; }  // not a tree in that order: no cones above
                b = below[size_t(ch)];
            } else {
                const uint32_t code = uint32_t(~ch), first = code >> 3, count = (code & 7u) + 1u;
                if (size_t(first) + count > n_tris) { all.sum[0] = kNaN; continue; }
                b.lo = first; b.hi = first + count; b.count = count;
                for (uint32_t t = first; t < first + count; t++)
                    for (int a = 0; a < 3; a++) b.sum[a] += normal[3 * size_t(t) + a];
            }
            (*out)[4 * i + size_t(k)] = cone_word(b);
            all.add(b);
        }
        below[i] = all;
    }
}

// ---------------------------------------------------------------------------------------------
// Normal slabs of the 4-wide mesh nodes.
//
// A child box is axis-aligned around a thin, tilted patch of surface: most rays that enter the box miss the patch.  Per child
// with a cone: q = the three axis bytes of its cone word as integers (no normalisation), s = 4 x the node's largest cell,
// P(x) = q . (x - org) / s, and [lo, hi] = the exact min / max of P over the corners v0, v0 + e1, v0 + e2 of every triangle
// below the child (over the triangles themselves, never a merge of the children's slabs), widened by the margin
// M = |q|_1 (2 m / s + 2^-12) (m = 2^-19 S, the pad of the mesh's boxes, S = its largest |coordinate|) and rounded outward to two
// signed 16-bit integers.  Inside the node |x_i - org_i| / s <= 63.75, so |P| <= 381 x 63.75 = 24 289: the scale holds every slab.
// P is linear, so every point of every triangle below lies in the slab.  k_wf_mesh evaluates, in f32,
//   r = (oc - org) / s, e = d / s, A = q . r, B = q . e, pn = fma(tn, B, A), pf = fma(tf, B, A)
// for the culling ray (oc, d) and the span [tn, tf] of the ray inside the child's box, and drops the child if pn and pf are
// both below lo or both above hi (rt_traverse.h node4q_cull_slabs).  Only a ray that the exact test would let hit a triangle
// below the child matters; for such a ray, with X the hit point and tau its parameter on the culling ray, u = 2^-24 and
// G = max_i(|org_i| / s, |r_i|, 128), in units of u |q|_1 G (1 / s is a power of two: scaling is exact):
//
//  1. oc in f32 is off by <= 2 u |oc_i| (one rounding in R, one to f32) and |oc_i| / s <= |org_i| / s + |r_i| <= 2 G: 4; the
//     subtraction of org adds u |r_i|: 1; the three-term chain of A adds 3 roundings of partial sums <= |q|_1 G: 3.  A: 8.
//  2. e is d rounded to f32 (u |e_i|), the chain of B adds 3 u sum |q_i e_i|; times t, where t |e_i| = |X_i - oc_i| / s
//     <= 64 + G <= 1.5 G for every t in [tn, tf] (both ends lie in the node's box): (1 + 3) x 1.5 = 6.
//  3. The last fma rounds a value <= |A| + |t B| <= 2.5 |q|_1 G: 2.5.
//  4. The culling ray itself (oc and d in f32) passes X within 2 u |oc_i| + u t |d_i|, over s: 4 + 1.5 = 5.5.
//     The step forms oc as fma(d, t_shift, o) (one rounding in R), make_cull_ray forms the origin that tn and tf are measured
//     from as o + d t_shift (two): the two starts differ by at most one rounding of R, u |oc_i| / s <= 2 more.
//  Together 24 u |q|_1 G.  For a ray that hits, oc and X lie in the mesh's box: |org_i| <= S, |r_i| <= 2 S / s, so
//  G <= max(2 S / s, 128) and 24 u |q|_1 G <= |q|_1 max(48 u S / s, 2^-12.4) <= M (2 m = 64 u S).  The 16 u S / s left over
//  cover tn and tf: the child's box holds X with the margin m on every side and the box test's own rounding is below
//  2.5 x 2^-23 S |iv| per plane (rt_tables.cpp), so tn <= tau <= tf; tau >= 0 up to one rounding of t_shift and
//  tau <= tmax32 by f32_at_least.  The function L(t) = A + t B with the COMPUTED A and B is exactly linear, so L(tau) lies
//  between L(tn) and L(tf), and L(tau) is within M of P(X), which lies in the unwidened slab: pn and pf cannot both be on the
//  same side outside [lo, hi].
//  This holds for R = double, where the exact test's own error (10 u_64, see the cones) is nothing against M.  It does NOT hold
//  for R = float: the f32 triangle test accepts rays whose u, v are off by an amount that grows with the distance of the ray's
//  origin from the triangle, that is, rays that pass the triangle farther off than M, and the slab - far tighter than the box -
//  drops them: 2 pixels of the f32 headline frame changed (profiles/mesh_slabs/README.md).  k_wf_mesh therefore has the step in
//  its f64 forms only; a slab for f32 needs a per-ray bound on that error first.  (The words are built for both types.)
//  5. Range: the kernel turns e into NaN unless 1e-20 < max |e_i| < 1e30 and G < 2^16, so no product overflows
//     (|B| <= 381 x 1e30), a flushed component of e moves t e_i by less than 2^17 x 1.2e-38 / 1e-20, and a bound clamped to
//     -32768 or 32767 is out of reach: |L(tau)| <= 24 289 + 24 u 381 x 2^16 < 24 325.  fmaxf / fminf drop a NaN operand: with
//     both ends NaN the comparisons fail; ONE NaN only arises as 0 x inf from tf = +inf and B = 0, where the true pf equals pn.
// The test does not read the direction word: it holds for meshes that hit back faces and with RT_WF_CONES=0.
// Nothing above depends on how q was chosen: it uses |q_i| <= 127 (the bytes), |q|_1 in the margin and in the scale bound, and
// the exact interval of P over the corners.  The axis need not be a normal at all, which is what build_mesh_slab_axes below uses.
// A child with kNeutralCone (empty, above an ill-conditioned triangle, a leaf without a cone, an inner child for which no axis of
// the table was worth taking) carries kNeutralSlab; its q is 0, so the kernel sees A = B = 0 (or NaN) inside [-32768, 32767] and
// never drops it.
// ---------------------------------------------------------------------------------------------
void build_mesh_slabs(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const std::vector<uint32_t>& cones,
                      const BvhNode4q* qnodes, const double* node_pad, std::vector<uint32_t>* out) {
    const size_t n_tris = tris.size();
    struct Run { uint32_t lo = UINT32_MAX, hi = 0, count = 0; };
    auto tri_at = [&](uint32_t t, double* v) {
        const TriRec<double>& r = tris[t];
        for (int a = 0; a < 3; a++) { v[a] = r.v0[a]; v[3 + a] = r.e1[a]; v[6 + a] = r.e2[a]; }
    };
    out->assign(4 * nodes4.size(), kNeutralSlab);
    std::vector<Run> below(nodes4.size());
    for (size_t i = nodes4.size(); i-- > 0;) {  // as build_mesh_cones
        const BuildNode4& nd = nodes4[i];
        Run all;
        for (int k = 0; k < 4; k++) {
            const int32_t ch = nd.child[k];
            if (ch == kEmptyChild) continue;
            Run b;
            if (ch >= 0) {
                if (size_t(ch) <= i || size_t(ch) >= nodes4.size()) continue;  // build_mesh_cones leaves no cone above: no slab either
                b = below[size_t(ch)];
            } else {
                const uint32_t code = uint32_t(~ch), first = code >> 3, count = (code & 7u) + 1u;
                if (size_t(first) + count > n_tris) continue;
                b.lo = first; b.hi = first + count; b.count = count;
            }
            (*out)[4 * i + size_t(k)] = rf_slab_word(cones[4 * i + size_t(k)], qnodes[i].org, qnodes[i].cell, node_pad[i], b.lo, b.hi, b.count, tri_at);
            all.lo = std::min(all.lo, b.lo); all.hi = std::max(all.hi, b.hi);
            all.count += b.count;
        }
        below[i] = all;
    }
}

// ---------------------------------------------------------------------------------------------
// Slab-only axes: a slab for inner children that have no back-face cone.
//
// The children of the top levels of a closed surface hold normals that go all the way round: no cone, so no axis, so no slab,
// although every mesh ray passes them and their boxes around bent pieces of surface are the loosest of the tree.  Such a child
// gets the word (qx, qy, qz, 127) with q from the table of rf_slab_axis (rt_refit.h): per candidate the exact extent of
// q . x over the corners below (v0, v0 + e1, v0 + e2, as the slabs form them) over the extent of the child's exact box along
// q, sum_a |q_a| (hi_a - lo_a); the candidate with the smallest ratio, the first of equals, if that ratio is below
// kSlabAxisMaxRatio.  build_mesh_slabs then gives it the slab of that axis like any other.
//
// The word never culls as a cone.  The kernel culls on D . (q, 127) > 0 with D = (dq, -127), that is dq . q > 127 x 127 = 16 129.
// Every byte of dq is round(127 d^_i) of a unit vector: |dq|_2 <= 127 + sqrt(3) / 2 < 127.87; every table entry has
// |q|_2 <= 126; so dq . q <= 127.87 x 126 < 16 112 < 16 129.  kNoCullDir has dq = 0: the product is -16 129.  The axis of a real
// cone is round(127 a), |a| = 1, of length >= 127 - sqrt(3) / 2 > 126: the two kinds of word cannot be confused, and
// rf_is_slab_only tells them apart.
// The slab proof above holds as it stands (it never asked where q came from).  Its scale bound: |P| <= |q|_1 x 63.75 with
// |q|_1 <= 216 for the table (72 + 72 + 72), below the 381 of a cone axis.
//
// Kept neutral: leaves (a leaf without a cone is a fold or a coincident pair; a slab there saves tests, not visits, and the
// work model shows none saved), children above an ill-conditioned triangle, children whose triangles are not one run of slots,
// children whose box is flat or not finite, and children whose slab on the chosen axis would be kNeutralSlab.
//
// Cost.  The supports are minima and maxima of identically computed numbers, so they merge exactly: a child's support is the
// merge of the supports of its own children, each of which is either computed by the recursion (it is eligible itself) or
// projected directly.  Every triangle is projected once per candidate however deep the stack of cone-less ancestors above it
// is (a triangle soup included), and the memory is one support per level of that stack.  (Skipping subtrees whose box cannot
// widen a support was tried: the deepest eligible children are small, most of their triangles are near their hull, 59 % of the
// headline mesh was still projected and the box tests cost what was saved.)  The refit kernel (rt_refit.hip k_refit_slab_axes)
// reduces over all corners of each eligible child instead; both give the exact minima and maxima, so the same words.
// ---------------------------------------------------------------------------------------------
bool slab_axes_enabled() {
    const char* e = std::getenv("RT_SLAB_AXES");
    return !(e && *e && std::atoi(e) == 0);
}

namespace {
struct AxisSupport {
    double lo[kSlabAxes], hi[kSlabAxes];
    AxisSupport() { for (int c = 0; c < kSlabAxes; c++) { lo[c] = INFINITY; hi[c] = -INFINITY; } }
    void merge(const AxisSupport& o) { for (int c = 0; c < kSlabAxes; c++) { lo[c] = rf_min(lo[c], o.lo[c]); hi[c] = rf_max(hi[c], o.hi[c]); } }
};

struct AxisPass {
    const std::vector<BuildNode4>& nodes4;
    const std::vector<TriRec<double>>& tris;
    const BvhNode4q* qnodes;
    const double* node_pad;
    std::vector<uint32_t>& cones;
    struct Run { uint32_t lo = UINT32_MAX, hi = 0, count = 0; };
    std::vector<Run> run;            // per node and child
    std::vector<uint8_t> eligible;   // per node and child
    std::vector<uint8_t> done;
    double ax[kSlabAxes], ay[kSlabAxes], az[kSlabAxes];  // the table as doubles (exact), one array per component

    // rf_axis_project of every corner of the slots [lo, hi) against every candidate, into *s.  The loop over the candidates is the
    // inner one, over plain arrays, so that the compiler can keep it in vector registers; the operations are rf_axis_project's
    // and rf_min / rf_max's, in their order.
    void project(uint32_t lo, uint32_t hi, AxisSupport* s) const {
        double mn[kSlabAxes], mx[kSlabAxes];
        for (int c = 0; c < kSlabAxes; c++) { mn[c] = s->lo[c]; mx[c] = s->hi[c]; }
        for (uint32_t t = lo; t < hi; t++) {
            const TriRec<double>& r = tris[t];
            double v[9];
            for (int a = 0; a < 3; a++) { v[a] = r.v0[a]; v[3 + a] = r.e1[a]; v[6 + a] = r.e2[a]; }
            for (int c3 = 0; c3 < 3; c3++) {
                double x[3];
                rf_tri_corner(v, c3, x);
                const double x0 = x[0], x1 = x[1], x2 = x[2];
                for (int c = 0; c < kSlabAxes; c++) {
                    const double p = ax[c] * x0 + ay[c] * x1 + az[c] * x2;
                    mn[c] = p < mn[c] ? p : mn[c];
                    mx[c] = p > mx[c] ? p : mx[c];
                }
            }
        }
        for (int c = 0; c < kSlabAxes; c++) { s->lo[c] = mn[c]; s->hi[c] = mx[c]; }
    }
    // the support of the eligible child k of node i, and its word
    void visit(size_t i, int k, AxisSupport* s) {
        const size_t id = 4 * i + size_t(k), c = size_t(nodes4[i].child[k]);
        done[id] = 1;
        for (int j = 0; j < 4; j++) {
            if (nodes4[c].child[j] == kEmptyChild) continue;
            if (eligible[4 * c + size_t(j)]) {
                AxisSupport below;
                visit(c, j, &below);
                s->merge(below);
            } else {
                project(run[4 * c + size_t(j)].lo, run[4 * c + size_t(j)].hi, s);
            }
        }
        const int pick = rf_slab_axis_pick(nodes4[i].lo[k], nodes4[i].hi[k], s->lo, s->hi);
        if (pick < 0) return;
        const uint32_t word = rf_slab_axis_word(pick);
        const Run& r = run[id];
        const uint32_t slab = rf_slab_word(word, qnodes[i].org, qnodes[i].cell, node_pad[i], r.lo, r.hi, r.count, [&](uint32_t t, double* v) {
            for (int a = 0; a < 3; a++) { v[a] = tris[t].v0[a]; v[3 + a] = tris[t].e1[a]; v[6 + a] = tris[t].e2[a]; }
        });
        if (slab != kNeutralSlab) cones[id] = word;
    }
};
}  // namespace

void build_mesh_slab_axes(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const ConeLimits& lim,
                          const BvhNode4q* qnodes, const double* node_pad, std::vector<uint32_t>* cones) {
    const size_t n = nodes4.size(), n_tris = tris.size();
    if (n == 0 || cones->size() != 4 * n) return;
    AxisPass p{nodes4, tris, qnodes, node_pad, *cones, {}, {}, {}, {}, {}, {}};
    for (int c = 0; c < kSlabAxes; c++) {
        int q[3];
        rf_slab_axis(c, q);
        p.ax[c] = double(q[0]); p.ay[c] = double(q[1]); p.az[c] = double(q[2]);
    }
    // ill-conditioned triangles before each slot, by the rule of build_mesh_cones
    std::vector<uint32_t> bad_before(n_tris + 1, 0);
    for (size_t t = 0; t < n_tris; t++) {
        double nrm[3];
        rf_tri_normal(tris[t].v0, tris[t].e1, tris[t].e2, lim, nrm);
        bad_before[t + 1] = bad_before[t] + (std::isfinite(nrm[0]) ? 0u : 1u);
    }
    p.run.resize(4 * n);
    p.eligible.assign(4 * n, 0);
    p.done.assign(4 * n, 0);
    for (size_t i = n; i-- > 0;) {  // runs, bottom-up as in build_mesh_slabs
        for (int k = 0; k < 4; k++) {
            const int32_t ch = nodes4[i].child[k];
            AxisPass::Run& b = p.run[4 * i + size_t(k)];
            if (ch == kEmptyChild) continue;
            if (ch >= 0) {
                if (size_t(ch) <= i || size_t(ch) >= n) continue;
                for (int j = 0; j < 4; j++) {
                    const AxisPass::Run& o = p.run[4 * size_t(ch) + size_t(j)];
                    b.lo = std::min(b.lo, o.lo); b.hi = std::max(b.hi, o.hi); b.count += o.count;
                }
                if (b.count == 0 || b.hi - b.lo != b.count || b.hi > n_tris) continue;
                const double clean[3] = {bad_before[b.hi] == bad_before[b.lo] ? 0.0 : std::numeric_limits<double>::quiet_NaN(), 0.0, 0.0};
                p.eligible[4 * i + size_t(k)] = rf_slab_axis_eligible(0, 1, (*cones)[4 * i + size_t(k)], b.lo, b.hi, b.count, clean) ? 1 : 0;
            } else {
                const uint32_t code = uint32_t(~ch), first = code >> 3, count = (code & 7u) + 1u;
                if (size_t(first) + count > n_tris) continue;
                b.lo = first; b.hi = first + count; b.count = count;
            }
        }
    }
    for (size_t i = 0; i < n; i++)  // parents stand before their children: an eligible child below an eligible one is done by then
        for (int k = 0; k < 4; k++)
            if (p.eligible[4 * i + size_t(k)] && !p.done[4 * i + size_t(k)]) {
                AxisSupport s;
                p.visit(i, k, &s);
            }
}

}  // namespace rt
