// lightmap_check.cpp — the texel rule of lightmaps on the host (csrc/rt_lightmap.h through rt_lightmap_texels_desc, rt_desc.cpp)
// as a stand-alone program, for sanitizer runs (no HIP include path: none of these files needs one):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o lightmap_check tools/lightmap_check.cpp
//       rust_raytracer_amd/csrc/rt_desc.cpp rust_raytracer_amd/csrc/rt_tables.cpp rust_raytracer_amd/csrc/rt_compile.cpp
//       rust_raytracer_amd/csrc/rt_bvh.cpp && ./lightmap_check
// A mesh of six triangles under a transform - a quad of two, a triangle that sticks out of the unit square, one without UV
// indices, one of zero UV area, one that overlaps the quad - rasterised into heap buffers of exactly width * height entries
// (an overrun is the sanitizer's report), with and without counts, at 7 x 5, 16 x 16, 33 x 1 and 1 x 1; every refusal with the
// outputs checked untouched; lm_dilate_texel over a 5 x 4 image.  Prints one summary line per map.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../rust_raytracer_amd/csrc/rt_desc.h"

namespace rt {  // the host builder is all this scene asks for
bool build_bvh_device(const double*, uint32_t, const uint32_t*, uint32_t, uint32_t, BvhBuild*, std::string* err) {
    *err = "no device builder in lightmap_check";
    return false;
}
}  // namespace rt

#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s failed (last error: %s)\n", __LINE__, #cond, rt_last_error()); return 1; } } while (0)

int main() {
    // positions = (u, v, 0.25 u v) of every corner; one normal
    const double uv[][2] = {{0.1, 0.1}, {0.9, 0.1}, {0.9, 0.9}, {0.1, 0.9},   // the quad
                            {0.5, 0.95}, {1.4, 0.95}, {0.5, 1.3},             // sticks out
                            {0.2, 0.2}, {0.4, 0.2}, {0.4, 0.4},               // no UV indices
                            {0.3, 0.3}, {0.5, 0.5}, {0.7, 0.7},               // zero area
                            {0.3, 0.2}, {0.8, 0.3}, {0.5, 0.8}};              // overlaps the quad
    const uint32_t n_pos = sizeof uv / sizeof uv[0];
    std::vector<double> positions, uvs;
    for (uint32_t i = 0; i < n_pos; i++) {
        positions.insert(positions.end(), {uv[i][0], uv[i][1], 0.25 * uv[i][0] * uv[i][1]});
        uvs.insert(uvs.end(), {uv[i][0], uv[i][1], 0.0});
    }
    const double normals[] = {0.0, 0.0, 1.0, 0.6, 0.0, 0.8};
    const uint32_t tri_pos[] = {0, 1, 2, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const uint32_t tri_nrm[] = {0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0};
    const int32_t tri_uv[] = {0, 1, 2, 0, 2, 3, 4, 5, 6, -1, -1, -1, 10, 11, 12, 13, 14, 15};
    RtMesh mesh{};
    mesh.positions = positions.data(); mesh.normals = normals; mesh.uvs = uvs.data();
    mesh.tri_pos = tri_pos; mesh.tri_nrm = tri_nrm; mesh.tri_uv = tri_uv;
    mesh.n_positions = n_pos; mesh.n_normals = 2; mesh.n_uvs = n_pos; mesh.n_triangles = 6;
    RtMesh bare = mesh;  // the same mesh without UVs
    bare.uvs = nullptr; bare.tri_uv = nullptr; bare.n_uvs = 0;
    const RtMesh meshes[] = {mesh, bare};

    RtTransform xf{};
    for (int i = 0; i < 4; i++) xf.m[5 * i] = xf.inv[5 * i] = 1.0;
    xf.m[0] = xf.m[5] = xf.m[10] = 2.0; xf.inv[0] = xf.inv[5] = xf.inv[10] = 0.5;
    xf.m[3] = 1.0; xf.m[7] = -2.0; xf.m[11] = 0.5;
    xf.inv[3] = -0.5; xf.inv[7] = 1.0; xf.inv[11] = -0.25;

    auto node = [](uint32_t type, double lo, double hi) {
        RtNode n{};
        n.type = type; n.material = -1; n.mesh = -1; n.transform = -1;
        for (int a = 0; a < 3; a++) { n.bounds[a] = lo; n.bounds[3 + a] = hi; }
        return n;
    };
    // 0: list (world), 1: transform -> 2: mesh 0, 3: mesh 1 (no UVs), 4: empty list (lights)
    RtNode nodes[5] = {node(RT_NODE_LIST, -10, 10), node(RT_NODE_TRANSFORM, -10, 10), node(RT_NODE_MESH, -1, 2), node(RT_NODE_MESH, -1, 2),
                       node(RT_NODE_LIST, 0, 0)};
    const uint32_t children[] = {1, 3, 2};
    nodes[0].first_child = 0; nodes[0].n_children = 2;
    nodes[1].first_child = 2; nodes[1].n_children = 1; nodes[1].transform = 0;
    nodes[2].mesh = 0; nodes[2].material = 0;
    nodes[3].mesh = 1; nodes[3].material = 0;
    RtMaterial mat{};
    mat.type = RT_MAT_LAMBERTIAN; mat.tex_a = 0; mat.tex_b = -1; mat.tex_c = -1;
    RtTexture tex{};
    tex.type = RT_TEX_CONST_COLOR; tex.a = tex.b = tex.c = -1; tex.v[0] = tex.v[1] = tex.v[2] = 0.7;
    RtSceneDesc d{};
    d.abi_version = RT_MI355_ABI_VERSION;
    d.n_nodes = 5; d.nodes = nodes; d.n_child_indices = 3; d.child_indices = children; d.n_transforms = 1; d.transforms = &xf;
    d.n_meshes = 2; d.meshes = meshes; d.n_materials = 1; d.materials = &mat; d.n_textures = 1; d.textures = &tex;
    d.world_root = 0; d.lights_root = 4;

    const uint32_t sizes[][2] = {{7, 5}, {16, 16}, {33, 1}, {1, 1}};
    for (const auto& s : sizes) {
        const uint32_t w = s[0], h = s[1];
        const size_t n = size_t(w) * h;
        std::unique_ptr<RtRayHit[]> hits(new RtRayHit[n]), hits2(new RtRayHit[n]);
        std::unique_ptr<uint32_t[]> counts(new uint32_t[n]);
        CHECK(rt_lightmap_texels_desc(&d, 2, 0, w, h, hits.get(), counts.get()) == RT_OK);
        CHECK(rt_lightmap_texels_desc(&d, 2, 0, w, h, hits2.get(), nullptr) == RT_OK);
        CHECK(std::memcmp(hits.get(), hits2.get(), n * sizeof(RtRayHit)) == 0);
        size_t covered = 0, twice = 0;
        double sum = 0.0;
        for (size_t i = 0; i < n; i++) {
            const RtRayHit& r = hits[i];
            CHECK((counts[i] > 0) == ((r.flags & RT_RAY_HIT) != 0));
            if (!counts[i]) { CHECK(r.prim == -1 && r.node == -1 && std::isinf(r.t)); continue; }
            covered++;
            twice += counts[i] > 1;
            CHECK(r.prim != 3 && r.prim != 4 && r.node == 2 && r.material == 0 && r.t == 0.0);
            CHECK(std::fabs(r.normal[0] * r.normal[0] + r.normal[1] * r.normal[1] + r.normal[2] * r.normal[2] - 1.0) < 1e-12);
            CHECK(std::fabs(r.pos[0] - (2.0 * r.u + 1.0)) < 1e-12 && std::fabs(r.pos[1] - (2.0 * r.v - 2.0)) < 1e-12);  // positions are the UVs
            sum += r.pos[2];
        }
        std::printf("%u x %u: %zu covered, %zu by more than one triangle, sum of z %.17g\n", w, h, covered, twice, sum);
    }

    // refusals: the outputs stay as they were
    RtRayHit guard[4];
    std::memset(guard, 0x5A, sizeof guard);
    uint32_t cguard[4] = {9, 9, 9, 9};
    auto untouched = [&]() {
        for (size_t i = 0; i < sizeof guard; i++)
            if (reinterpret_cast<const unsigned char*>(guard)[i] != 0x5A) return false;
        return cguard[0] == 9 && cguard[1] == 9 && cguard[2] == 9 && cguard[3] == 9;
    };
    CHECK(rt_lightmap_texels_desc(&d, 2, 0, 0, 2, guard, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 2, 0, 2, 16385, guard, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 5, 0, 2, 2, guard, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 1, 0, 2, 2, guard, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 2, 1, 2, 2, guard, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 3, 0, 2, 2, guard, cguard) == RT_E_UNSUPPORTED && untouched());
    CHECK(rt_lightmap_texels_desc(&d, 2, 0, 2, 2, nullptr, cguard) == RT_E_INVALID && untouched());
    CHECK(rt_lightmap_texels_desc(nullptr, 2, 0, 2, 2, guard, cguard) == RT_E_INVALID && untouched());

    // dilation of one pass over a 5 x 4 image in heap buffers of exactly its size
    const uint32_t w = 5, h = 4;
    std::unique_ptr<double[]> img(new double[w * h * 4]), out(new double[w * h * 4]);
    std::unique_ptr<uint8_t[]> cov(new uint8_t[w * h]), cov_out(new uint8_t[w * h]);
    for (uint32_t i = 0; i < w * h; i++) {
        cov[i] = (i % 7 == 0) ? 1 : 0;
        for (int k = 0; k < 4; k++) img[4 * i + k] = double(i) + 0.25 * k;
    }
    uint32_t filled = 0;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            rt::lm_dilate_texel(img.get(), cov.get(), w, h, x, y, out.get() + 4 * (size_t(y) * w + x), cov_out.get() + size_t(y) * w + x);
            filled += cov_out[size_t(y) * w + x] && !cov[size_t(y) * w + x];
        }
    std::printf("dilation: %u texels filled in one pass\n", filled);
    std::printf("ok\n");
    return 0;
}
