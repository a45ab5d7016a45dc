// tables_check.cpp — the host derivation of the kernels' tables (rt_tables.cpp) as a stand-alone program, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o tables_check tools/tables_check.cpp
//       rust_raytracer_amd/csrc/rt_tables.cpp rust_raytracer_amd/csrc/rt_compile.cpp rust_raytracer_amd/csrc/rt_bvh.cpp && ./tables_check
// A cube mesh instanced twice under two transforms, a second mesh (a tetrahedron), a sphere and a quad in a list; prints the
// seven table digests (the order of rt_scene_tables_digest) in both precisions.
#include <cstdio>

#include "../rust_raytracer_amd/csrc/rt_tables.h"

namespace rt {  // the host builder is all this scene asks for
bool build_bvh_device(const double*, uint32_t, const uint32_t*, uint32_t, uint32_t, BvhBuild*, std::string* err) {
    *err = "no device builder in tables_check";
    return false;
}
}  // namespace rt

static RtNode node(uint32_t type, int32_t material, double lo, double hi) {
    RtNode n{};
    n.type = type; n.material = material; n.mesh = -1; n.transform = -1;
    for (int a = 0; a < 3; a++) { n.bounds[a] = lo; n.bounds[3 + a] = hi; }
    return n;
}
static RtTransform translate(double x, double y, double z) {
    RtTransform t{};
    for (int i = 0; i < 4; i++) t.m[5 * i] = t.inv[5 * i] = 1.0;
    t.m[3] = x; t.m[7] = y; t.m[11] = z;
    t.inv[3] = -x; t.inv[7] = -y; t.inv[11] = -z;
    return t;
}
template <typename R>
static int print_digests(const rt::CompiledScene& cs, const char* name) {
    rt::MeshTables<R> m;
    rt::SceneTables<R> t;
    std::string err;
    if (rt::derive_mesh_tables(cs, &m, &err) != RT_OK || rt::derive_scene_tables(cs, &t, &err) != RT_OK) { std::printf("%s\n", err.c_str()); return 1; }
    std::printf("%s", name);
    for (const auto& tbl : rt::digest_tables(cs, m, t)) {
        rt::Digest g;
        g.bytes(tbl.first, tbl.second);
        std::printf(" %016llx", (unsigned long long)g.value());
    }
    std::printf("\n");
    return 0;
}

int main() {
    const double cube_p[24] = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1};
    const uint32_t cube_t[36] = {0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 6, 2, 3, 7, 6, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5};
    const double tet_p[12] = {2, 0, 0, 5, 0.5, 0, 3, 4, 1, 3, 1, 6};
    const uint32_t tet_t[12] = {0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2};
    const double up[3] = {0, 1, 0};
    const uint32_t nrm[36] = {};
    RtMesh meshes[2] = {};
    meshes[0].positions = cube_p; meshes[0].n_positions = 8; meshes[0].tri_pos = cube_t; meshes[0].n_triangles = 12;
    meshes[1].positions = tet_p; meshes[1].n_positions = 4; meshes[1].tri_pos = tet_t; meshes[1].n_triangles = 4;
    for (RtMesh& m : meshes) { m.normals = up; m.n_normals = 1; m.tri_nrm = nrm; }
    RtTexture tex{};
    tex.type = RT_TEX_CONST_COLOR; tex.a = tex.b = tex.c = -1; tex.v[0] = tex.v[1] = tex.v[2] = 0.7;
    const RtMaterial mat{RT_MAT_LAMBERTIAN, 0, -1, -1, 1.5};
    const RtTransform xf[2] = {translate(-3, 0, 0), translate(0.5, 2, -4)};
    // 0, 1: the cube twice; 2, 3: their transforms; 4: the tetrahedron; 5: sphere; 6: quad; 7: their list; 8: world
    RtNode nodes[9] = {node(RT_NODE_MESH, 0, 0, 1), node(RT_NODE_MESH, 0, 0, 1), node(RT_NODE_TRANSFORM, -1, -3, 3), node(RT_NODE_TRANSFORM, -1, -4, 3),
                       node(RT_NODE_MESH, 0, 0, 6), node(RT_NODE_SPHERE, 0, -2, 0), node(RT_NODE_PLANE, 0, -1, 1), node(RT_NODE_LIST, -1, -2, 1),
                       node(RT_NODE_LIST, -1, -4, 6)};
    nodes[0].mesh = nodes[1].mesh = 0; nodes[4].mesh = 1;
    const uint32_t kids[8] = {0, 1, 5, 6, 2, 3, 4, 7};
    nodes[2].transform = 0; nodes[2].first_child = 0; nodes[2].n_children = 1;
    nodes[3].transform = 1; nodes[3].first_child = 1; nodes[3].n_children = 1;
    nodes[5].p[0] = nodes[5].p[1] = nodes[5].p[2] = -1; nodes[5].p[3] = 1;
    nodes[6].p[3] = 1; nodes[6].p[8] = 1;  // centre 0, u = x, v = z
    nodes[7].first_child = 2; nodes[7].n_children = 2;
    nodes[8].first_child = 4; nodes[8].n_children = 4;
    RtSceneDesc d{};
    d.abi_version = RT_MI355_ABI_VERSION;
    d.nodes = nodes; d.n_nodes = 9; d.child_indices = kids; d.n_child_indices = 8; d.transforms = xf; d.n_transforms = 2;
    d.meshes = meshes; d.n_meshes = 2; d.materials = &mat; d.n_materials = 1; d.textures = &tex; d.n_textures = 1;
    d.world_root = 8; d.lights_root = 7;
    rt::CompiledScene cs;
    std::string err;
    if (rt::compile_scene(&d, &cs, &err) != RT_OK) { std::printf("compile_scene: %s\n", err.c_str()); return 1; }
    std::printf("%zu mesh instances, %zu distinct meshes, %zu 4-wide nodes, %zu triangles\n", cs.meshes.size(), cs.mesh_geoms.size(), cs.nodes4.size(), cs.tris.size());
    return print_digests<double>(cs, "f64") | print_digests<float>(cs, "f32");
}
