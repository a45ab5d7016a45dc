// tables_check.cpp — the host derivation of the kernels' tables (rt_tables.cpp) and the description-only entry points of the C
// ABI (rt_desc.cpp) as a stand-alone program, for sanitizer runs (no HIP include path: none of these files needs one):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o tables_check tools/tables_check.cpp
//       rust_raytracer_amd/csrc/rt_desc.cpp rust_raytracer_amd/csrc/rt_tables.cpp rust_raytracer_amd/csrc/rt_compile.cpp
//       rust_raytracer_amd/csrc/rt_bvh.cpp && ./tables_check
// A cube mesh instanced twice under two transforms, a second mesh (a tetrahedron), a sphere and a quad in a list; prints the
// seven table digests (the order of rt_scene_tables_digest) in both precisions.  Then the exports of rt_desc.cpp into heap
// buffers of exactly the reported sizes and of one entry less (an overrun is the sanitizer's report; the shorter result
// must be a prefix of the full one), rt_scene_update_check, HeldDesc after its sources are freed, the host half of
// rt_scene_update, rt_light_groups_auto and rt_debug_handout_replay.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../rust_raytracer_amd/csrc/rt_desc.h"

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

// ---- the description-only entry points (rt_desc.cpp): every output in a heap buffer of exactly its size ----
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s failed (last error: %s)\n", __LINE__, #cond, rt_last_error()); return 1; } } while (0)
template <typename T>
struct Heap {
    size_t n;
    std::unique_ptr<T[]> p;
    explicit Heap(size_t n_) : n(n_), p(new T[n_]()) {}
    Heap(const T* src, size_t n_) : n(n_), p(new T[n_]) { std::copy(src, src + n_, p.get()); }
    T* get() const { return p.get(); }
    bool prefix_of(const Heap& full) const { return n <= full.n && std::memcmp(p.get(), full.p.get(), n * sizeof(T)) == 0; }
};
static uint32_t less(uint32_t n) { return n ? n - 1 : 0; }  // the truncated capacity

// d: the scene of main(); d2: the same with the tetrahedron's vertices moved
static int check_exports(const RtSceneDesc& d, const RtSceneDesc& d2) {
    for (uint32_t f32 = 0; f32 < 2; f32++)
        for (uint32_t mesh = 0; mesh < 3; mesh++) {
            uint32_t nn = 0, nt = 0, n2 = 0, t2 = 0;
            CHECK(rt_scene_refit_mesh(&d, &d2, mesh, f32, nullptr, nullptr, nullptr, 0, &nn, nullptr, nullptr, 0, &nt) == RT_OK && nn && nt);
            {  // exact sizes, then one less
                Heap<int32_t> ch(4 * size_t(nn)), ch1(4 * size_t(less(nn)));
                Heap<uint32_t> co(4 * size_t(nn)), co1(4 * size_t(less(nn))), ord(nt), ord1(less(nt));
                Heap<float> bx(24 * size_t(nn)), bx1(24 * size_t(less(nn)));
                Heap<double> tr(9 * size_t(nt)), tr1(9 * size_t(less(nt)));
                CHECK(rt_scene_refit_mesh(&d, &d2, mesh, f32, ch.get(), co.get(), bx.get(), nn, &n2, tr.get(), ord.get(), nt, &t2) == RT_OK && n2 == nn && t2 == nt);
                CHECK(rt_scene_refit_mesh(&d, &d2, mesh, f32, ch1.get(), co1.get(), bx1.get(), less(nn), &n2, tr1.get(), ord1.get(), less(nt), &t2) == RT_OK && n2 == nn && t2 == nt);
                CHECK(ch1.prefix_of(ch) && co1.prefix_of(co) && bx1.prefix_of(bx) && tr1.prefix_of(tr) && ord1.prefix_of(ord));
            }
            uint32_t cnn = 0, cnt = 0;
            CHECK(rt_scene_mesh_cones(&d, mesh, f32, nullptr, nullptr, 0, &cnn, nullptr, 0, &cnt) == RT_OK && cnn == nn && cnt == nt);
            Heap<int32_t> ch(4 * size_t(nn)), ch1(4 * size_t(less(nn)));
            Heap<uint32_t> co(4 * size_t(nn)), co1(4 * size_t(less(nn)));
            Heap<double> tr(9 * size_t(nt)), tr1(9 * size_t(less(nt)));
            CHECK(rt_scene_mesh_cones(&d, mesh, f32, ch.get(), co.get(), nn, &cnn, tr.get(), nt, &cnt) == RT_OK && cnn == nn && cnt == nt);
            CHECK(rt_scene_mesh_cones(&d, mesh, f32, ch1.get(), co1.get(), less(nn), &cnn, tr1.get(), less(nt), &cnt) == RT_OK && cnn == nn && cnt == nt);
            CHECK(ch1.prefix_of(ch) && co1.prefix_of(co) && tr1.prefix_of(tr));
            uint32_t snn = 0;
            double pad = 0.0, pad1 = 0.0;
            CHECK(rt_scene_mesh_slabs(&d, mesh, f32, nullptr, nullptr, nullptr, nullptr, 0, &snn) == RT_OK && snn == nn);
            Heap<uint32_t> sl(4 * size_t(nn)), sl1(4 * size_t(less(nn)));
            Heap<float> bo(8 * size_t(nn)), bo1(8 * size_t(less(nn))), fr(4 * size_t(nn)), fr1(4 * size_t(less(nn)));
            CHECK(rt_scene_mesh_slabs(&d, mesh, f32, sl.get(), bo.get(), fr.get(), &pad, nn, &snn) == RT_OK && snn == nn);
            CHECK(rt_scene_mesh_slabs(&d, mesh, f32, sl1.get(), bo1.get(), fr1.get(), &pad1, less(nn), &snn) == RT_OK && snn == nn);
            CHECK(sl1.prefix_of(sl) && bo1.prefix_of(bo) && fr1.prefix_of(fr) && pad == pad1 && pad > 0.0);
            if (f32 == 0) std::printf("mesh instance %u: %u nodes, %u triangles\n", mesh, nn, nt);
        }
    uint32_t n_ops = 0, n_ops2 = 0;
    uint64_t info[8], info2[8];
    CHECK(rt_scene_program(&d, nullptr, 0, &n_ops, info) == RT_OK && n_ops);
    Heap<int32_t> ops(4 * size_t(n_ops)), ops1(4 * size_t(less(n_ops)));
    CHECK(rt_scene_program(&d, ops.get(), n_ops, &n_ops2, info2) == RT_OK && n_ops2 == n_ops && std::memcmp(info, info2, sizeof info) == 0);
    CHECK(rt_scene_program(&d, ops1.get(), less(n_ops), &n_ops2, info2) == RT_OK && n_ops2 == n_ops && ops1.prefix_of(ops));
    CHECK(rt_scene_op_nodes(&d, nullptr, 0, &n_ops2) == RT_OK && n_ops2 == n_ops);
    Heap<int32_t> on(n_ops), on1(less(n_ops));
    CHECK(rt_scene_op_nodes(&d, on.get(), n_ops, &n_ops2) == RT_OK && n_ops2 == n_ops);
    CHECK(rt_scene_op_nodes(&d, on1.get(), less(n_ops), &n_ops2) == RT_OK && n_ops2 == n_ops && on1.prefix_of(on));
    std::printf("program: %u ops, %llu mesh ops, %llu lights\n", n_ops, (unsigned long long)info[0], (unsigned long long)info[4]);
    return 0;
}

// rt_scene_groups on a scene that has a group: a list of 14 spheres, one of which touches the list's box (a guard)
static int check_groups() {
    RtNode nodes[15];
    uint32_t kids[14];
    for (uint32_t i = 0; i < 14; i++) {
        nodes[i] = node(RT_NODE_SPHERE, 0, -8, 8);
        nodes[i].p[0] = double(i % 4) * 2.0 - 3.0; nodes[i].p[1] = double(i / 4) * 2.0 - 3.0; nodes[i].p[2] = double(i % 3); nodes[i].p[3] = 0.5 + 0.125 * double(i % 2);
        kids[i] = i;
    }
    nodes[13].p[0] = 7.5; nodes[13].p[3] = 0.5;  // reaches x = 8, the face of the list's box
    nodes[14] = node(RT_NODE_LIST, -1, -8, 8);
    nodes[14].first_child = 0; nodes[14].n_children = 14;
    RtTexture tex{};
    tex.type = RT_TEX_CONST_COLOR; tex.a = tex.b = tex.c = -1; tex.v[0] = tex.v[1] = tex.v[2] = 0.7;
    const RtMaterial mat{RT_MAT_LAMBERTIAN, 0, -1, -1, 1.5};
    RtSceneDesc d{};
    d.abi_version = RT_MI355_ABI_VERSION;
    d.nodes = nodes; d.n_nodes = 15; d.child_indices = kids; d.n_child_indices = 14;
    d.materials = &mat; d.n_materials = 1; d.textures = &tex; d.n_textures = 1;
    d.world_root = 14; d.lights_root = 14;
    for (uint32_t f32 = 0; f32 < 2; f32++) {
        uint32_t c[6] = {}, c2[6] = {};
        CHECK(rt_scene_groups(&d, f32, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, c) == RT_OK);
        CHECK(c[0] == 1 && c[1] >= 1 && c[2] == 14 && c[3] >= 1);
        Heap<uint32_t> ro(c[0]), ro1(less(c[0]));
        Heap<double> gb(6 * size_t(c[0])), gb1(6 * size_t(less(c[0])));
        Heap<int32_t> ch(4 * size_t(c[1])), ch1(4 * size_t(less(c[1]))), pr(3 * size_t(c[2])), pr1(3 * size_t(less(c[2]))), gu(c[3]), gu1(less(c[3]));
        Heap<float> bx(24 * size_t(c[1])), bx1(24 * size_t(less(c[1])));
        CHECK(rt_scene_groups(&d, f32, ro.get(), gb.get(), c[0], ch.get(), bx.get(), c[1], pr.get(), c[2], gu.get(), c[3], c2) == RT_OK && std::memcmp(c, c2, sizeof c) == 0);
        CHECK(rt_scene_groups(&d, f32, ro1.get(), gb1.get(), less(c[0]), ch1.get(), bx1.get(), less(c[1]), pr1.get(), less(c[2]), gu1.get(), less(c[3]), c2) == RT_OK &&
              std::memcmp(c, c2, sizeof c) == 0);
        CHECK(ro1.prefix_of(ro) && gb1.prefix_of(gb) && ch1.prefix_of(ch) && bx1.prefix_of(bx) && pr1.prefix_of(pr) && gu1.prefix_of(gu));
        if (f32 == 0) std::printf("groups: %u groups, %u nodes, %u primitives, %u guards\n", c[0], c[1], c[2], c[3]);
    }
    return 0;
}

static int check_update_check(const RtSceneDesc& d) {
    CHECK(rt_scene_update_check(&d, &d) == RT_OK);
    RtMesh meshes[2] = {d.meshes[0], d.meshes[1]};
    RtSceneDesc e = d;
    e.meshes = meshes;
    meshes[1].n_triangles--;
    CHECK(rt_scene_update_check(&d, &e) == RT_E_INVALID && std::strstr(rt_last_error(), "meshes[1].n_triangles"));
    meshes[1].n_triangles++;
    Heap<uint32_t> tri(d.meshes[0].tri_pos, 3 * size_t(d.meshes[0].n_triangles));
    tri.get()[tri.n - 1] ^= 1u;
    meshes[0].tri_pos = tri.get();
    CHECK(rt_scene_update_check(&d, &e) == RT_E_INVALID && std::strstr(rt_last_error(), "meshes[0].tri_pos"));
    std::printf("update_check: %s\n", rt_last_error());
    return 0;
}

// The sum of every array a description reaches (transforms apart: a HeldDesc keeps none)
static double desc_sum(const RtSceneDesc& d) {
    double s = 0.0;
    for (uint32_t i = 0; i < d.n_nodes; i++) {
        for (double b : d.nodes[i].bounds) s += b;
        for (double p : d.nodes[i].p) s += p;
        s += d.nodes[i].type + d.nodes[i].first_child;
    }
    for (uint32_t i = 0; i < d.n_child_indices; i++) s += d.child_indices[i];
    for (uint32_t i = 0; i < d.n_meshes; i++) {
        const RtMesh& m = d.meshes[i];
        for (size_t k = 0; k < 3 * size_t(m.n_positions); k++) s += m.positions[k];
        for (size_t k = 0; k < 3 * size_t(m.n_normals); k++) s += m.normals[k];
        for (size_t k = 0; m.uvs && k < 3 * size_t(m.n_uvs); k++) s += m.uvs[k];
        for (size_t k = 0; k < 3 * size_t(m.n_triangles); k++) s += m.tri_pos[k] + m.tri_nrm[k] + (m.tri_uv ? m.tri_uv[k] : 0);
    }
    for (uint32_t i = 0; i < d.n_materials; i++) s += d.materials[i].ior + d.materials[i].type;
    for (uint32_t i = 0; i < d.n_textures; i++) s += d.textures[i].v[0] + d.textures[i].type;
    return s;
}
// a mesh whose arrays all live in heap buffers of their own
struct HeapMesh {
    Heap<double> positions, normals;
    Heap<uint32_t> tri_pos, tri_nrm;
    explicit HeapMesh(const RtMesh& m) : positions(m.positions, 3 * size_t(m.n_positions)), normals(m.normals, 3 * size_t(m.n_normals)),
                                         tri_pos(m.tri_pos, 3 * size_t(m.n_triangles)), tri_nrm(m.tri_nrm, 3 * size_t(m.n_triangles)) {}
    RtMesh mesh(RtMesh m) const { m.positions = positions.get(); m.normals = normals.get(); m.tri_pos = tri_pos.get(); m.tri_nrm = tri_nrm.get(); return m; }
};
static int check_held_desc(const RtSceneDesc& d, const double* tet_moved) {
    rt::HeldDesc held;
    {
        const HeapMesh h0(d.meshes[0]), h1(d.meshes[1]);
        const RtMesh meshes[2] = {h0.mesh(d.meshes[0]), h1.mesh(d.meshes[1])};
        RtSceneDesc first = d;
        first.meshes = meshes;
        held.assign(first);
    }  // the first description's arrays are gone
    double want;
    {
        RtMesh moved = d.meshes[1];
        moved.positions = tet_moved;
        const HeapMesh h1(moved);
        const RtMesh meshes[2] = {d.meshes[0], h1.mesh(moved)};
        RtSceneDesc second = d;
        second.meshes = meshes;
        want = desc_sum(second);
        const std::vector<bool> keep = {true, false};
        rt::HeldDesc old = std::move(held);  // as rt_scene_update commits
        held.assign(second, &old, &keep);
    }  // ... and so are the second's and the old copy
    const double got = desc_sum(held.d);
    CHECK(got == want && held.d.n_meshes == 2 && held.d.transforms == nullptr);
    std::printf("held description: sum %.17g\n", got);
    return 0;
}

static int check_update_plan(const RtSceneDesc& d, const rt::CompiledScene& cs, const RtSceneDesc& d2) {
    rt::HeldDesc held;
    held.assign(d);
    rt::UpdatePlan same, moved, refused;
    CHECK(rt::plan_scene_update(held, cs, &d, &same) == RT_OK && same.moved.empty() && same.n_tris_moved == 0);
    CHECK(rt::plan_scene_update(held, cs, &d2, &moved) == RT_OK && moved.moved.size() == 1 && cs.mesh_geoms[moved.moved[0]].mesh == 1 && moved.n_tris_moved == 4);
    CHECK(moved.changed == std::vector<bool>({false, true}) && moved.same == std::vector<bool>({true, false}) && moved.cs.tris.size() == cs.tris.size());
    Heap<double> nan_p(d.meshes[1].positions, 12);
    nan_p.get()[7] = std::nan("");
    RtMesh meshes[2] = {d.meshes[0], d.meshes[1]};
    meshes[1].positions = nan_p.get();
    RtSceneDesc e = d;
    e.meshes = meshes;
    CHECK(rt::plan_scene_update(held, cs, &e, &refused) == RT_E_UNSUPPORTED &&
          !std::strcmp(rt_last_error(), "scene update: meshes[1].positions: coordinates beyond the f32 grid"));
    std::printf("update plan: %zu mesh moved, %u triangles; NaN: %s\n", moved.moved.size(), moved.n_tris_moved, rt_last_error());
    return 0;
}

static int check_light_groups(const RtSceneDesc& d) {
    Heap<uint8_t> group(d.n_materials);
    Heap<uint32_t> out(2);
    CHECK(rt_light_groups_auto(&d, RT_LIGHT_GROUPS_MAX, 1, group.get(), out.get(), out.get() + 1) == RT_OK);
    std::printf("light groups: material 0 in group %u, background in group %u, %u groups\n", group.get()[0], out.get()[0], out.get()[1]);
    return 0;
}

static int check_handout() {
    const Heap<uint32_t> order(3);
    for (uint32_t g = 0; g < 3; g++) order.get()[g] = g;
    Heap<uint32_t> n_asks(2), atomics(2), atomics2(2);
    CHECK(rt_debug_handout_replay(nullptr, 1000, 3, order.get(), 3, nullptr, 0, n_asks.get(), atomics.get()) == RT_OK && n_asks.get()[0]);
    Heap<uint32_t> asks(3 * size_t(n_asks.get()[0]));
    CHECK(rt_debug_handout_replay(nullptr, 1000, 3, order.get(), 3, asks.get(), n_asks.get()[0], n_asks.get() + 1, atomics2.get()) == RT_OK);
    CHECK(n_asks.get()[1] == n_asks.get()[0] && atomics2.prefix_of(atomics));
    uint32_t served = 0;
    for (uint32_t i = 0; i < n_asks.get()[0]; i++)
        if (asks.get()[3 * i + 1] != 0xFFFFFFFFu) served += asks.get()[3 * i + 2] - asks.get()[3 * i + 1];
    CHECK(served == 1000);
    std::printf("handout: %u asks, %u + %u atomics, %u entries served\n", n_asks.get()[0], atomics.get()[0], atomics.get()[1], served);
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
    if (print_digests<double>(cs, "f64") | print_digests<float>(cs, "f32")) return 1;
    // the same description with the tetrahedron moved: what rt_scene_update is given
    double tet_moved[12];
    for (int i = 0; i < 12; i++) tet_moved[i] = tet_p[i] + 0.25 * (i % 3);
    RtMesh meshes2[2] = {meshes[0], meshes[1]};
    meshes2[1].positions = tet_moved;
    RtSceneDesc d2 = d;
    d2.meshes = meshes2;
    return check_exports(d, d2) || check_groups() || check_update_check(d) || check_held_desc(d, tet_moved) || check_update_plan(d, cs, d2) ||
           check_light_groups(d) || check_handout();
}
