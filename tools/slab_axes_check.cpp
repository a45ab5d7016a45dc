// slab_axes_check.cpp — the slab-only axes pass of the host builder (rt_bvh.cpp build_mesh_slab_axes) as a stand-alone program, for
// sanitizer runs and for timing the pass:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Irust_raytracer_amd/csrc -o slab_axes_check
//       tools/slab_axes_check.cpp rust_raytracer_amd/csrc/rt_bvh.cpp rust_raytracer_amd/csrc/rt_tables.cpp && ./slab_axes_check a.obj b.obj ...
// Per OBJ file and conditioning limit (f64, f32): build_bvh, collapse_bvh4, the cones, the axes, the slabs; checks that the pass only
// turns neutral words of inner children into slab-only words that have a slab, and prints the counts and the time of each part.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_bvh.h"
#include "rt_refit.h"
#include "rt_scene.h"

using namespace rt;

static bool load_obj(const char* path, std::vector<double>* pos, std::vector<uint32_t>* tri) {
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    char line[512];
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == 'v' && line[1] == ' ') {
            double x, y, z;
            if (std::sscanf(line + 2, "%lf %lf %lf", &x, &y, &z) == 3) { pos->push_back(x); pos->push_back(y); pos->push_back(z); }
        } else if (line[0] == 'f' && line[1] == ' ') {
            unsigned idx[3];
            int n = 0;
            for (char* p = line + 2; *p && n < 3;) {
                while (*p == ' ') p++;
                if (*p < '0' || *p > '9') break;
                idx[n++] = unsigned(std::strtoul(p, &p, 10));
                while (*p && *p != ' ') p++;
            }
            if (n == 3) for (int k = 0; k < 3; k++) tri->push_back(idx[k] - 1);
        }
    }
    std::fclose(f);
    for (uint32_t i : *tri) if (size_t(i) * 3 + 2 >= pos->size()) return false;
    return !tri->empty();
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int arg = 1; arg < argc; arg++) {
        std::vector<double> pos;
        std::vector<uint32_t> tri;
        if (!load_obj(argv[arg], &pos, &tri)) { std::printf("%s: cannot read triangles\n", argv[arg]); return 1; }
        const uint32_t nt = uint32_t(tri.size() / 3);
        const BvhBuild bvh = build_bvh(pos.data(), tri.data(), nt, 4);
        const Bvh4Build b4 = collapse_bvh4(bvh);
        std::vector<TriRec<double>> tris(nt);
        for (uint32_t s = 0; s < nt; s++) {
            const uint32_t t = bvh.tri_order[s];
            const double *p0 = &pos[3 * size_t(tri[3 * size_t(t)])], *p1 = &pos[3 * size_t(tri[3 * size_t(t) + 1])], *p2 = &pos[3 * size_t(tri[3 * size_t(t) + 2])];
            for (int a = 0; a < 3; a++) { tris[s].v0[a] = p0[a]; tris[s].e1[a] = p1[a] - p0[a]; tris[s].e2[a] = p2[a] - p0[a]; }
        }
        const double pad = rf_pad_of_box(b4.root_lo, b4.root_hi);
        const std::vector<double> node_pad(b4.nodes.size(), pad);
        std::vector<BvhNode4q> qnodes(b4.nodes.size());
        for (size_t i = 0; i < qnodes.size(); i++) {
            for (int k = 0; k < 4; k++) qnodes[i].child[k] = b4.nodes[i].child[k];
            if (!rf_quantise4(b4.nodes[i].lo, b4.nodes[i].hi, b4.nodes[i].child, pad, qnodes[i].org, qnodes[i].cell, qnodes[i].qlo, qnodes[i].qhi)) {
                std::printf("%s: a node does not fit the grid\n", argv[arg]);
                return 1;
            }
        }
        for (int f32 = 0; f32 < 2; f32++) {
            std::vector<uint32_t> cones, before, slabs;
            auto t0 = std::chrono::steady_clock::now();
            build_mesh_cones(b4.nodes, tris, cone_limits(f32 != 0), &cones);
            const double ms_cones = ms_since(t0);
            before = cones;
            t0 = std::chrono::steady_clock::now();
            build_mesh_slab_axes(b4.nodes, tris, cone_limits(f32 != 0), qnodes.data(), node_pad.data(), &cones);
            const double ms_axes = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            build_mesh_slabs(b4.nodes, tris, cones, qnodes.data(), node_pad.data(), &slabs);
            const double ms_slabs = ms_since(t0);
            size_t inner_neutral = 0, fitted = 0;
            for (size_t i = 0; i < b4.nodes.size(); i++)
                for (int k = 0; k < 4; k++) {
                    const size_t id = 4 * i + size_t(k);
                    const int32_t c = b4.nodes[i].child[k];
                    if (c >= 0 && before[id] == kNeutralCone) inner_neutral++;
                    if (cones[id] == before[id]) continue;
                    fitted++;
                    if (!(c >= 0 && before[id] == kNeutralCone && rf_is_slab_only(cones[id]) && slabs[id] != kNeutralSlab)) {
                        std::printf("%s: child %d of node %zu: word %08x -> %08x, slab %08x\n", argv[arg], k, i, before[id], cones[id], slabs[id]);
                        bad++;
                    }
                }
            std::printf("%s %s: %u triangles, %zu nodes, %zu inner children without a cone, %zu with a slab-only axis; cones %.1f ms, axes %.1f ms, slabs %.1f ms\n",
                        argv[arg], f32 ? "f32" : "f64", nt, b4.nodes.size(), inner_neutral, fitted, ms_cones, ms_axes, ms_slabs);
        }
    }
    return bad ? 2 : 0;
}
