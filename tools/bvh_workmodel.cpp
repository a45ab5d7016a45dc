// CPU work model of k_wf_mesh: node visits and triangle tests per mesh ray of the 4-wide BVH the kernel walks, with and
// without the back-face cone test and the normal-slab test, on a small path tracer of scenes/cornell_dragon.  Host only; built by hand:
//
//   g++ -std=c++17 -O2 -Irust_raytracer_amd/csrc -o tools/bvh_workmodel tools/bvh_workmodel.cpp rust_raytracer_amd/csrc/rt_bvh.cpp rust_raytracer_amd/csrc/rt_tables.cpp
//   tools/bvh_workmodel scenes/resource/dragon_high.obj [paths = 150000] [pad0]
//
// The tables are derived twice by the library itself: with RT_SLAB_AXES=0 (cones and the slabs on their axes: the rows "with
// cones" and "+ slabs") and with the slab-only axes of inner children without a cone (rt_bvh.cpp build_mesh_slab_axes: the row
// "+ fitted axes").  For the last row it also prints the visits per depth of the tree and the split of the mesh rays by where
// they start (on the mesh: the ray leaves a mesh hit; elsewhere) and whether they hit.
//
// pad0: the slab words are built with the mesh pad m = 0, which leaves of the margin |q|_1 (2 m / s + 2^-12) only the constant
// term (below 0.1 of the 16-bit step): what the slabs could be worth with no margin at all.  Such words are NOT safe for the kernel.
//
// It links the repository's own build_bvh / collapse_bvh4 / build_mesh_cones / build_mesh_slabs (the slab words are the
// library's: same axis bytes, same 16-bit encoding, same margin; the step is node4q_cull_slabs restated in f32) and walks the tree exactly as the kernel
// does: four slab tests per node, children sorted by entry distance, far children pushed, entries culled on pop, every
// triangle of a leaf tested with the reference's front-face rule.  The boxes are exact here (the kernel's 8-bit boxes
// add about 2 % to the visits of every tree alike).  With exact boxes it reproduces the counters of the headline
// workload (bench.py --workload c4 --full: node_visits_per_ray, tri_tests_per_ray; per ray = per mesh ray x the share of
// mesh rays that it prints).  It is the cheap way to judge a builder, collapse, leaf size or culling idea before any
// kernel is touched: change the tree or the traversal here and compare the two numbers.  The cone test must also leave
// every ray's closest hit unchanged (same triangle, same t): the model counts the rays for which it does not.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include <cstring>

#include "rt_bvh.h"
#include "rt_refit.h"
#include "rt_scene.h"
#include "rt_tables.h"

using namespace rt;
static const double kInf = std::numeric_limits<double>::infinity();

struct V { double x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return a * (1.0 / std::sqrt(dot(a, a))); }

struct Mesh { std::vector<double> pos; std::vector<uint32_t> tri; };
// "v x y z" and triangular "f a[/b[/c]] ..." lines
static bool load_obj(const char* path, Mesh* m) {
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    char line[512];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == 'v' && line[1] == ' ') {
            double x, y, z;
            if (std::sscanf(line + 2, "%lf %lf %lf", &x, &y, &z) == 3) { m->pos.push_back(x); m->pos.push_back(y); m->pos.push_back(z); }
        } else if (line[0] == 'f' && line[1] == ' ') {
            unsigned idx[3];
            int n = 0;
            for (char* p = line + 2; *p && n < 3;) {
                while (*p == ' ') p++;
                if (*p < '0' || *p > '9') break;
                idx[n++] = unsigned(std::strtoul(p, &p, 10));
                while (*p && *p != ' ') p++;
            }
            if (n == 3) for (int k = 0; k < 3; k++) m->tri.push_back(idx[k] - 1);
        }
    }
    std::fclose(f);
    return !m->tri.empty();
}

constexpr int kDepths = 12;  // deeper nodes count into the last bin
struct Counters {
    unsigned long long rays = 0, visits = 0, tests = 0, hits = 0;
    unsigned long long by_depth[kDepths] = {};
    void add(const Counters& o) {
        rays += o.rays; visits += o.visits; tests += o.tests; hits += o.hits;
        for (int i = 0; i < kDepths; i++) by_depth[i] += o.by_depth[i];
    }
};
static std::vector<uint8_t> g_depth;  // per node: levels below the root

// The slab tables of the tree: words and quantised nodes (grid origin, cells); mode 0 off, 1 every child, 2 leaf children only.
struct Slabs { const uint32_t* words; const BvhNode4q* qnodes; int mode; double t_shift; };

// node4q_cull_slabs of rt_traverse.h for one child, in f32: true if the span [tn, tf] (measured from o + d t_shift) lies
// wholly outside the child's slab.
static bool slab_culls(const Slabs& sl, size_t node, int k, uint32_t cone, V o, V d, float tn, float tf) {
    const BvhNode4q& q = sl.qnodes[node];
    const float cmax = std::fmax(std::fmax(q.cell[0], q.cell[1]), q.cell[2]);
    uint32_t cb;
    std::memcpy(&cb, &cmax, 4);
    cb = 0x7E000000u - cb;
    float inv_s;
    std::memcpy(&inv_s, &cb, 4);
    const float rx = (float(std::fma(d.x, sl.t_shift, o.x)) - q.org[0]) * inv_s, ry = (float(std::fma(d.y, sl.t_shift, o.y)) - q.org[1]) * inv_s,
                rz = (float(std::fma(d.z, sl.t_shift, o.z)) - q.org[2]) * inv_s;
    float ex = float(d.x) * inv_s;
    const float ey = float(d.y) * inv_s, ez = float(d.z) * inv_s;
    const float em = std::fmax(std::fmax(std::fabs(ex), std::fabs(ey)), std::fabs(ez));
    const float gm = std::fmax(std::fmax(std::fmax(std::fabs(q.org[0]), std::fabs(q.org[1])), std::fabs(q.org[2])) * inv_s,
                               std::fmax(std::fmax(std::fabs(rx), std::fabs(ry)), std::fabs(rz)));
    if (!(em > 1e-20f && em < 1e30f && gm < 65536.0f)) ex = NAN;
    const float qx = float(int8_t(cone & 0xFF)), qy = float(int8_t((cone >> 8) & 0xFF)), qz = float(int8_t((cone >> 16) & 0xFF));
    const float A = std::fmaf(qx, rx, std::fmaf(qy, ry, qz * rz)), B = std::fmaf(qx, ex, std::fmaf(qy, ey, qz * ez));
    const float pn = std::fmaf(tn, B, A), pf = std::fmaf(tf, B, A);
    const uint32_t w = sl.words[4 * node + size_t(k)];
    const float lo = float(int16_t(w & 0xFFFFu)), hi = float(int16_t(w >> 16));
    return std::fmax(pn, pf) < lo || std::fmin(pn, pf) > hi;
}

// Closest hit in (0.001, tmax) as k_wf_mesh finds it.  cones: 4 words per node, or nullptr; sl: the slab test, or nullptr.
static bool traverse(const Bvh4Build& b, const std::vector<TriRec<double>>& tris, const uint32_t* cones, const Slabs* sl, V o, V d, double tmax,
                     Counters& c, double* t_out, int* tri_out) {
    const V du = unit(d);
    const int dq[3] = {int(std::lround(du.x * 127)), int(std::lround(du.y * 127)), int(std::lround(du.z * 127))};
    const V iv = {1.0 / d.x, 1.0 / d.y, 1.0 / d.z};
    struct Entry { int32_t child; double t; };
    std::vector<Entry> stack;
    int32_t node = 0;
    int hit = -1;
    c.rays++;
    for (;;) {
        bool descend = false;
        if (node >= 0) {
            c.visits++;
            c.by_depth[std::min<int>(g_depth[size_t(node)], kDepths - 1)]++;
            const BuildNode4& n = b.nodes[size_t(node)];
            double nr[4];
            int32_t ch[4];
            for (int k = 0; k < 4; k++) {
                ch[k] = n.child[k];
                nr[k] = kInf;
                if (ch[k] == kEmptyChild) continue;
                if (cones) {  // dir . cone > 0: every triangle below faces away
                    const uint32_t w = cones[4 * size_t(node) + size_t(k)];
                    const int prod = dq[0] * int8_t(w & 0xFF) + dq[1] * int8_t((w >> 8) & 0xFF) + dq[2] * int8_t((w >> 16) & 0xFF) - 127 * int8_t(w >> 24);
                    if (prod > 0) continue;
                }
                double t0x = (n.lo[k][0] - o.x) * iv.x, t1x = (n.hi[k][0] - o.x) * iv.x; if (t0x > t1x) std::swap(t0x, t1x);
                double t0y = (n.lo[k][1] - o.y) * iv.y, t1y = (n.hi[k][1] - o.y) * iv.y; if (t0y > t1y) std::swap(t0y, t1y);
                double t0z = (n.lo[k][2] - o.z) * iv.z, t1z = (n.hi[k][2] - o.z) * iv.z; if (t0z > t1z) std::swap(t0z, t1z);
                const double tn = std::max(std::max(t0x, t0y), std::max(t0z, 0.0)), tf = std::min(std::min(t1x, t1y), std::min(t1z, tmax));
                if (tn <= tf) nr[k] = tn;
                if (tn <= tf && sl && sl->mode != 0 && (sl->mode == 1 || ch[k] < 0) &&
                    slab_culls(*sl, size_t(node), k, cones[4 * size_t(node) + size_t(k)], o, d, float(tn - sl->t_shift), float(tf - sl->t_shift)))
                    nr[k] = kInf;  // the entry distances of the others stay what they are
            }
            auto ce = [&](int a, int bb) { if (nr[a] > nr[bb]) { std::swap(nr[a], nr[bb]); std::swap(ch[a], ch[bb]); } };
            ce(0, 1); ce(2, 3); ce(0, 2); ce(1, 3); ce(1, 2);
            if (nr[0] < kInf) {
                for (int k = 3; k >= 1; k--) if (nr[k] < kInf) stack.push_back({ch[k], nr[k]});
                node = ch[0];
                descend = true;
            }
        } else {
            const uint32_t code = uint32_t(~node), first = code >> 3, count = (code & 7u) + 1u;
            for (uint32_t j = 0; j < count; j++) {
                c.tests++;
                const TriRec<double>& tr = tris[first + j];
                const V e1 = {tr.e1[0], tr.e1[1], tr.e1[2]}, e2 = {tr.e2[0], tr.e2[1], tr.e2[2]}, v0 = {tr.v0[0], tr.v0[1], tr.v0[2]};
                const V p = cross(d, e2);
                const double det = dot(e1, p);
                if (det < std::numeric_limits<double>::epsilon()) continue;  // mesh.rs:77
                const double inv = 1.0 / det;
                const V s = o - v0;
                const double u = dot(s, p) * inv;
                if (u < 0 || u > 1) continue;
                const V q = cross(s, e1);
                const double v = dot(d, q) * inv;
                if (v < 0 || u + v > 1) continue;
                const double t = dot(e2, q) * inv;
                if (t <= 0.001 || tmax <= t) continue;
                tmax = t;
                hit = int(first + j);
            }
        }
        if (descend) continue;
        bool found = false;
        while (!stack.empty()) {
            const Entry e = stack.back();
            stack.pop_back();
            if (e.t <= tmax) { node = e.child; found = true; break; }
        }
        if (!found) break;
    }
    if (hit < 0) return false;
    c.hits++;
    *t_out = tmax;
    *tri_out = hit;
    return true;
}

// SplitMix64
struct Rng {
    uint64_t s;
    double u() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return double(z >> 11) * (1.0 / 9007199254740992.0);
    }
};
static V cosine_dir(V n, Rng& r) {
    const double u1 = r.u(), u2 = r.u(), ph = 2 * M_PI * u1, sr = std::sqrt(u2);
    const V a = std::fabs(n.x) > 0.9 ? V{0, 1, 0} : V{1, 0, 0};
    const V t = unit(cross(n, a)), bt = cross(n, t);
    return unit(t * (std::cos(ph) * sr) + bt * (std::sin(ph) * sr) + n * std::sqrt(1 - u2));
}

int main(int argc, char** argv) {
    Mesh m;
    const char* path = argc > 1 ? argv[1] : "scenes/resource/dragon_high.obj";
    if (!load_obj(path, &m)) { std::fprintf(stderr, "cannot read triangles from %s\n", path); return 1; }
    const uint32_t nt = uint32_t(m.tri.size() / 3);
    const int n_paths = argc > 2 ? std::atoi(argv[2]) : 150000;

    const BvhBuild bvh = build_bvh(m.pos.data(), m.tri.data(), nt, 4);
    const Bvh4Build b4 = collapse_bvh4(bvh);
    std::vector<TriRec<double>> tris(nt);
    for (uint32_t s = 0; s < nt; s++) {
        const uint32_t t = bvh.tri_order[s];
        const double* p0 = &m.pos[3 * size_t(m.tri[3 * size_t(t)])];
        const double* p1 = &m.pos[3 * size_t(m.tri[3 * size_t(t) + 1])];
        const double* p2 = &m.pos[3 * size_t(m.tri[3 * size_t(t) + 2])];
        for (int a = 0; a < 3; a++) { tris[s].v0[a] = p0[a]; tris[s].e1[a] = p1[a] - p0[a]; tris[s].e2[a] = p2[a] - p0[a]; }
    }
    // the quantised nodes with their cone and slab words: the library's own derivation (rt_tables.cpp) over a one-mesh scene
    CompiledScene scene;
    scene.nodes4 = b4.nodes;
    scene.tris = tris;
    scene.meshes.push_back(MeshInst{});
    Bounds<double> box;
    for (int a = 0; a < 3; a++) { box.lo[a] = b4.root_lo[a]; box.hi[a] = b4.root_hi[a]; }
    scene.mesh_bounds.push_back(box);
    scene.mesh_geoms.push_back(CompiledScene::MeshGeom{0, 0, 0, 0, uint32_t(b4.nodes.size()), 0, nt, bvh.max_depth, b4.max_stack});
    MeshTables<double> tables, tables_fit;
    std::string err;
    auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double derive_ms[2][3];  // derive_mesh_tables without / with the slab-only axes, three times each, alternating
    for (int rep = 0; rep < 3; rep++) {
        setenv("RT_SLAB_AXES", "0", 1);
        double t0 = now_ms();
        if (derive_mesh_tables(scene, &tables, &err) != RT_OK) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        derive_ms[0][rep] = now_ms() - t0;
        unsetenv("RT_SLAB_AXES");
        t0 = now_ms();
        if (derive_mesh_tables(scene, &tables_fit, &err) != RT_OK) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        derive_ms[1][rep] = now_ms() - t0;
    }
    std::vector<BvhNode4q> qnodes(b4.nodes.size());
    std::vector<uint32_t> cones(4 * b4.nodes.size()), slab_words(4 * b4.nodes.size()), cones_fit(4 * b4.nodes.size()), slab_words_fit(4 * b4.nodes.size());
    for (size_t i = 0; i < b4.nodes.size(); i++) {
        qnodes[i] = tables.nodes4qc[i].node;
        for (int k = 0; k < 4; k++) {
            cones[4 * i + size_t(k)] = tables.nodes4qc[i].cones.word[k]; slab_words[4 * i + size_t(k)] = tables.nodes4qc[i].slabs.word[k];
            cones_fit[4 * i + size_t(k)] = tables_fit.nodes4qc[i].cones.word[k]; slab_words_fit[4 * i + size_t(k)] = tables_fit.nodes4qc[i].slabs.word[k];
        }
    }
    const bool pad0 = argc > 3 && std::strcmp(argv[3], "pad0") == 0;
    if (pad0) {  // the experiment: leaves the library's margin on purpose
        const std::vector<double> zero(b4.nodes.size(), 0.0);
        build_mesh_slabs(b4.nodes, tris, cones, qnodes.data(), zero.data(), &slab_words);
        build_mesh_slabs(b4.nodes, tris, cones_fit, qnodes.data(), zero.data(), &slab_words_fit);
    }
    g_depth.assign(b4.nodes.size(), 0);
    for (size_t i = 0; i < b4.nodes.size(); i++)  // children stand behind their parent
        for (int k = 0; k < 4; k++) {
            const int32_t c = b4.nodes[i].child[k];
            if (c >= 0 && size_t(c) < b4.nodes.size()) g_depth[size_t(c)] = uint8_t(std::min(255, g_depth[i] + 1));
        }
    size_t fitted = 0;
    for (size_t i = 0; i < cones_fit.size(); i++) fitted += rf_is_slab_only(cones_fit[i]) ? 1 : 0;
    size_t with_slab = 0, with_cone = 0;
    for (size_t i = 0; i < slab_words.size(); i++) { with_slab += slab_words[i] != kNeutralSlab; with_cone += cones[i] != kNeutralCone; }
    size_t leaf = 0, leaf_cone = 0, inner = 0, inner_cone = 0;
    for (size_t i = 0; i < b4.nodes.size(); i++)
        for (int k = 0; k < 4; k++) {
            const int32_t c = b4.nodes[i].child[k];
            if (c == kEmptyChild) continue;
            const bool has = cones[4 * i + size_t(k)] != kNeutralCone;
            if (c < 0) { leaf++; leaf_cone += has; } else { inner++; inner_cone += has; }
        }
    std::printf("%u triangles, %zu 4-wide nodes (depth %u, stack %u); cones on %zu of %zu leaf children (%.2f %%), %zu of %zu inner children (%.2f %%)\n",
                nt, b4.nodes.size(), b4.max_depth, b4.max_stack, leaf_cone, leaf, 100.0 * leaf_cone / std::max<size_t>(leaf, 1), inner_cone, inner,
                100.0 * inner_cone / std::max<size_t>(inner, 1));

    // scenes/cornell_dragon: five lambertian walls, a light in the ceiling, the mesh under s=60 ry=225 t=267.5,0.5,277.5 (half
    // mirror, half cosine bounces: the glossy material with roughness 0 does either); the mesh is traced in object space
    const double th = 225.0 * M_PI / 180.0, cs = std::cos(th), sn = std::sin(th), S = 60.0;
    const V T = {267.5, 0.5, 277.5};
    auto to_obj_p = [&](V p) { const V q = p - T; return V{cs * q.x - sn * q.z, q.y, sn * q.x + cs * q.z} * (1.0 / S); };
    auto to_obj_d = [&](V d) { return V{cs * d.x - sn * d.z, d.y, sn * d.x + cs * d.z} * (1.0 / S); };
    auto to_world_d = [&](V d) { return V{cs * d.x + sn * d.z, d.y, -sn * d.x + cs * d.z}; };
    std::printf("slabs on %zu of the %zu children with a cone%s; slab-only axes on %zu of the %zu inner children without a cone (%d candidates, ratio below %.2f)\n",
                with_slab, with_cone, pad0 ? " (pad0: margin without the mesh pad)" : "", fitted, inner - inner_cone, kSlabAxes, kSlabAxisMaxRatio);
    std::printf("derive_mesh_tables<double>: %.0f / %.0f / %.0f ms with RT_SLAB_AXES=0, %.0f / %.0f / %.0f ms with the axes\n", derive_ms[0][0], derive_ms[0][1],
                derive_ms[0][2], derive_ms[1][0], derive_ms[1][1], derive_ms[1][2]);
    Counters plain, coned, plain_hit, plain_miss, slab_leaf, slab_all, slab_fit, fit_split[2][2];
    unsigned long long total_rays = 0, mesh_rays = 0, changed = 0, changed_leaf = 0, changed_all = 0, changed_fit = 0;
    bool on_mesh = false;  // the ray starts at a mesh hit
    Rng rng{12345};
    for (int p = 0; p < n_paths; p++) {
        V o = {277.5, 277.5, -800};
        on_mesh = false;
        V d = unit(V{rng.u() * 555.0, rng.u() * 555.0, 0} - o);
        for (int depth = 0; depth < 12; depth++) {
            total_rays++;
            double tw = kInf;
            V nw{0, 0, 0};
            auto plane = [&](double num, double den, V nrm) {
                if (std::fabs(den) < 1e-12) return;
                const double t = num / den;
                if (!(t > 0.001 && t < tw)) return;
                const V h = o + d * t;
                if (h.x >= -1e-6 && h.x <= 555 + 1e-6 && h.y >= -1e-6 && h.y <= 555 + 1e-6 && h.z >= -1e-6 && h.z <= 555 + 1e-6) { tw = t; nw = nrm; }
            };
            plane(0 - o.x, d.x, {1, 0, 0}); plane(555 - o.x, d.x, {-1, 0, 0}); plane(0 - o.y, d.y, {0, 1, 0}); plane(555 - o.y, d.y, {0, -1, 0});
            plane(555 - o.z, d.z, {0, 0, -1});
            const V oo = to_obj_p(o), od = to_obj_d(d);
            // a mesh ray is one that enters the mesh's box inside (0.001, tw), as k_wf_prims decides it
            double t0 = 0.001, t1 = tw;
            const double oa[3] = {oo.x, oo.y, oo.z}, da[3] = {od.x, od.y, od.z};
            for (int a = 0; a < 3; a++) {
                double x0 = (b4.root_lo[a] - oa[a]) / da[a], x1 = (b4.root_hi[a] - oa[a]) / da[a];
                if (x0 > x1) std::swap(x0, x1);
                t0 = std::max(t0, x0);
                t1 = std::min(t1, x1);
            }
            double t_hit = tw;
            int tri = -1;
            bool mesh_hit = false;
            if (t0 <= t1) {
                mesh_rays++;
                Counters one;
                mesh_hit = traverse(b4, tris, nullptr, nullptr, oo, od, tw, one, &t_hit, &tri);
                Counters& split = mesh_hit ? plain_hit : plain_miss;
                for (Counters* dst : {&plain, &split}) { dst->rays++; dst->visits += one.visits; dst->tests += one.tests; dst->hits += one.hits; }
                double t2 = tw;
                int tri2 = -1;
                const bool h2 = traverse(b4, tris, cones.data(), nullptr, oo, od, tw, coned, &t2, &tri2);
                if (h2 != mesh_hit || (h2 && (tri2 != tri || t2 != t_hit))) changed++;
                for (int mode = 2; mode >= 1; mode--) {
                    const Slabs sl{slab_words.data(), qnodes.data(), mode, std::max(t0, 0.0)};  // the culling ray starts where the ray enters the box
                    double t3 = tw;
                    int tri3 = -1;
                    const bool h3 = traverse(b4, tris, cones.data(), &sl, oo, od, tw, mode == 2 ? slab_leaf : slab_all, &t3, &tri3);
                    if (h3 != mesh_hit || (h3 && (tri3 != tri || t3 != t_hit))) (mode == 2 ? changed_leaf : changed_all)++;
                }
                {
                    const Slabs sl{slab_words_fit.data(), qnodes.data(), 1, std::max(t0, 0.0)};
                    double t4 = tw;
                    int tri4 = -1;
                    Counters one_fit;
                    const bool h4 = traverse(b4, tris, cones_fit.data(), &sl, oo, od, tw, one_fit, &t4, &tri4);
                    if (h4 != mesh_hit || (h4 && (tri4 != tri || t4 != t_hit))) changed_fit++;
                    slab_fit.add(one_fit);
                    fit_split[on_mesh ? 1 : 0][mesh_hit ? 1 : 0].add(one_fit);
                }
            }
            if (mesh_hit) {
                const TriRec<double>& tr = tris[size_t(tri)];
                V n = unit(to_world_d(cross(V{tr.e1[0], tr.e1[1], tr.e1[2]}, V{tr.e2[0], tr.e2[1], tr.e2[2]})));
                if (dot(n, d) > 0) n = n * -1.0;
                o = o + d * t_hit;
                on_mesh = true;
                d = rng.u() < 0.5 ? unit(d - n * (2 * dot(d, n))) : cosine_dir(n, rng);
            } else if (tw < kInf) {
                const V h = o + d * tw;
                if (nw.y < 0 && std::fabs(h.x - 277.5) < 130 && std::fabs(h.z - 277.5) < 105) break;  // the light
                o = h;
                on_mesh = false;
                d = cosine_dir(nw, rng);
            } else {
                break;
            }
        }
    }
    auto per = [](unsigned long long a, unsigned long long b) { return b ? double(a) / double(b) : 0.0; };
    std::printf("%d paths, %llu rays, %llu mesh rays (%.3f of all rays)\n", n_paths, total_rays, mesh_rays, per(mesh_rays, total_rays));
    std::printf("without cones: %6.2f visits, %6.2f tests per mesh ray (rays that hit: %.2f / %.2f, rays that miss: %.2f / %.2f)\n", per(plain.visits, plain.rays),
                per(plain.tests, plain.rays), per(plain_hit.visits, plain_hit.rays), per(plain_hit.tests, plain_hit.rays), per(plain_miss.visits, plain_miss.rays),
                per(plain_miss.tests, plain_miss.rays));
    std::printf("with cones:    %6.2f visits (%+.1f %%), %6.2f tests (%+.1f %%) per mesh ray; rays whose closest hit changed: %llu\n", per(coned.visits, coned.rays),
                100.0 * (per(coned.visits, plain.visits) - 1.0), per(coned.tests, coned.rays), 100.0 * (per(coned.tests, plain.tests) - 1.0), changed);
    std::printf("+ slabs, leaf children: %6.2f visits (%+.1f %% of cones), %6.2f tests (%+.1f %%) per mesh ray; rays whose closest hit changed: %llu\n",
                per(slab_leaf.visits, slab_leaf.rays), 100.0 * (per(slab_leaf.visits, coned.visits) - 1.0), per(slab_leaf.tests, slab_leaf.rays),
                100.0 * (per(slab_leaf.tests, coned.tests) - 1.0), changed_leaf);
    std::printf("+ slabs, every child:   %6.2f visits (%+.1f %% of cones), %6.2f tests (%+.1f %%) per mesh ray; rays whose closest hit changed: %llu\n",
                per(slab_all.visits, slab_all.rays), 100.0 * (per(slab_all.visits, coned.visits) - 1.0), per(slab_all.tests, slab_all.rays),
                100.0 * (per(slab_all.tests, coned.tests) - 1.0), changed_all);
    std::printf("+ fitted axes, every child: %6.2f visits (%+.1f %% of slabs on every child), %6.2f tests (%+.1f %%) per mesh ray; rays whose closest hit changed: %llu\n",
                per(slab_fit.visits, slab_fit.rays), 100.0 * (per(slab_fit.visits, slab_all.visits) - 1.0), per(slab_fit.tests, slab_fit.rays),
                100.0 * (per(slab_fit.tests, slab_all.tests) - 1.0), changed_fit);
    std::printf("visits per mesh ray by depth (root = 0), slabs on every child -> + fitted axes:");
    for (int i = 0; i < kDepths; i++) std::printf(" %d: %.2f -> %.2f;", i, per(slab_all.by_depth[i], slab_all.rays), per(slab_fit.by_depth[i], slab_fit.rays));
    std::printf("\nmesh rays with fitted axes by origin and outcome (share, visits, tests per ray):\n");
    const char* names[2][2] = {{"origin elsewhere, miss", "origin elsewhere, hit"}, {"origin on the mesh, miss", "origin on the mesh, hit"}};
    for (int a = 0; a < 2; a++)
        for (int h = 0; h < 2; h++)
            std::printf("  %-26s %5.1f %%  %6.2f  %6.2f   (%.1f %% of the visits)\n", names[a][h], 100.0 * per(fit_split[a][h].rays, slab_fit.rays),
                        per(fit_split[a][h].visits, fit_split[a][h].rays), per(fit_split[a][h].tests, fit_split[a][h].rays),
                        100.0 * per(fit_split[a][h].visits, slab_fit.visits));
    return (changed || changed_leaf || changed_all || changed_fit) ? 2 : 0;
}
