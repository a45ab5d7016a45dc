// rt_desc.cpp — the entry points of the C ABI (include/rt_mi355.h) that take a description and no scene: they compile it on
// the host, derive tables on the host (rt_tables.cpp) and copy numbers out.  Plain C++, no HIP: tools/tables_check.cpp runs
// them under sanitizers.
#include "rt_desc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_handout.h"
#include "rt_refit.h"

namespace rt {

// "Same structure, new numbers" (include/rt_mi355.h, rt_scene_update): empty if `b` has the structure of `a`, else a message
// that names the first field that differs.
static std::string update_mismatch(const RtSceneDesc& a, const RtSceneDesc& b) {
    auto idx = [](const char* table, uint32_t i, const char* field) { return std::string(table) + "[" + std::to_string(i) + "]." + field; };
#define RT_SAME(field) if (a.field != b.field) return std::string(#field)
    RT_SAME(n_nodes); RT_SAME(n_child_indices); RT_SAME(n_transforms); RT_SAME(n_meshes); RT_SAME(n_materials); RT_SAME(n_textures);
    RT_SAME(world_root); RT_SAME(lights_root);
#undef RT_SAME
    if ((b.n_nodes && !b.nodes) || (b.n_child_indices && !b.child_indices) || (b.n_transforms && !b.transforms) || (b.n_meshes && !b.meshes) ||
        (b.n_materials && !b.materials) || (b.n_textures && !b.textures))
        return "a table pointer is NULL";
    if (a.n_child_indices && std::memcmp(a.child_indices, b.child_indices, size_t(a.n_child_indices) * 4) != 0) return "child_indices";
#define RT_SAME(table, field) if (x.field != y.field) return idx(table, i, #field)
    for (uint32_t i = 0; i < a.n_nodes; i++) {
        const RtNode &x = a.nodes[i], &y = b.nodes[i];
        RT_SAME("nodes", type); RT_SAME("nodes", flags); RT_SAME("nodes", material); RT_SAME("nodes", mesh); RT_SAME("nodes", transform);
        RT_SAME("nodes", first_child); RT_SAME("nodes", n_children);
    }
    for (uint32_t i = 0; i < a.n_meshes; i++) {
        const RtMesh &x = a.meshes[i], &y = b.meshes[i];
        RT_SAME("meshes", n_positions); RT_SAME("meshes", n_normals); RT_SAME("meshes", n_uvs); RT_SAME("meshes", n_triangles); RT_SAME("meshes", flags);
        if (!x.positions != !y.positions) return idx("meshes", i, "positions");
        if (!x.normals != !y.normals) return idx("meshes", i, "normals");
        if (!x.uvs != !y.uvs) return idx("meshes", i, "uvs");
        if (!x.tri_pos != !y.tri_pos) return idx("meshes", i, "tri_pos");
        if (!x.tri_nrm != !y.tri_nrm) return idx("meshes", i, "tri_nrm");
        if (!x.tri_uv != !y.tri_uv) return idx("meshes", i, "tri_uv");
        const size_t nb = size_t(x.n_triangles) * 12;
        if (x.tri_pos && std::memcmp(x.tri_pos, y.tri_pos, nb) != 0) return idx("meshes", i, "tri_pos");
        if (x.tri_nrm && std::memcmp(x.tri_nrm, y.tri_nrm, nb) != 0) return idx("meshes", i, "tri_nrm");
        if (x.tri_uv && std::memcmp(x.tri_uv, y.tri_uv, nb) != 0) return idx("meshes", i, "tri_uv");
    }
    for (uint32_t i = 0; i < a.n_materials; i++) {
        const RtMaterial &x = a.materials[i], &y = b.materials[i];
        RT_SAME("materials", type); RT_SAME("materials", tex_a); RT_SAME("materials", tex_b); RT_SAME("materials", tex_c);
    }
    for (uint32_t i = 0; i < a.n_textures; i++) {
        const RtTexture &x = a.textures[i], &y = b.textures[i];
        RT_SAME("textures", type); RT_SAME("textures", a); RT_SAME("textures", b); RT_SAME("textures", c); RT_SAME("textures", channel);
        RT_SAME("textures", samples); RT_SAME("textures", width); RT_SAME("textures", height);
        if (!x.texels != !y.texels) return idx("textures", i, "texels");
        if (!x.perlin_vec != !y.perlin_vec) return idx("textures", i, "perlin_vec");
        if (!x.perlin_perm != !y.perlin_perm) return idx("textures", i, "perlin_perm");
    }
#undef RT_SAME
    return std::string();
}
static std::string update_mismatch_message(const std::string& field) {
    return "scene update: the description has another structure than the scene (first difference: " + field + ")";
}

uint64_t scene_digest(const RtSceneDesc& d) {
    Digest g;
    g.val(d.n_nodes); g.val(d.world_root); g.val(d.lights_root);
    for (uint32_t i = 0; i < d.n_nodes; i++) {
        const RtNode& n = d.nodes[i];
        g.val(n.type); g.val(n.flags); g.val(n.material); g.val(n.mesh); g.val(n.transform); g.val(n.first_child);
        g.val(n.n_children); g.val(n.bounds); g.val(n.p);
    }
    g.bytes(d.child_indices, size_t(d.n_child_indices) * 4);
    g.bytes(d.transforms, size_t(d.n_transforms) * sizeof(RtTransform));
    for (uint32_t i = 0; i < d.n_meshes; i++) {
        const RtMesh& m = d.meshes[i];
        g.val(m.n_positions); g.val(m.n_normals); g.val(m.n_uvs); g.val(m.n_triangles); g.val(m.flags);
        g.bytes(m.positions, size_t(m.n_positions) * 24);
        g.bytes(m.normals, size_t(m.n_normals) * 24);
        g.bytes(m.uvs, m.uvs ? size_t(m.n_uvs) * 24 : 0);
        g.bytes(m.tri_pos, size_t(m.n_triangles) * 12);
        g.bytes(m.tri_nrm, size_t(m.n_triangles) * 12);
        g.bytes(m.tri_uv, m.tri_uv ? size_t(m.n_triangles) * 12 : 0);
    }
    for (uint32_t i = 0; i < d.n_materials; i++) {
        const RtMaterial& m = d.materials[i];
        g.val(m.type); g.val(m.tex_a); g.val(m.tex_b); g.val(m.tex_c); g.val(m.ior);
    }
    for (uint32_t i = 0; i < d.n_textures; i++) {
        const RtTexture& t = d.textures[i];
        g.val(t.type); g.val(t.a); g.val(t.b); g.val(t.c); g.val(t.channel); g.val(t.samples); g.val(t.v); g.val(t.scale);
        g.val(t.width); g.val(t.height);
        g.bytes(t.texels, t.texels ? size_t(t.width) * t.height * 3 * sizeof(float) : 0);
        g.bytes(t.perlin_vec, t.perlin_vec ? 256 * 3 * sizeof(double) : 0);
        g.bytes(t.perlin_perm, t.perlin_perm ? 3 * 256 * sizeof(uint32_t) : 0);
    }
    return g.value();
}

uint32_t owned_rows(uint32_t h, const RtRenderParams* p) {
    if (p->band_rows == 0 || p->n_parts <= 1) return h;
    uint32_t n = 0;
    for (uint32_t y = 0; y < h; y++)
        if ((y / p->band_rows) % p->n_parts == p->part) n++;
    return n;
}

// The scene compiler's switches (every entry point that compiles a description reads them the same way).
static CompileOptions compile_options_from_env() {
    CompileOptions opt;
    if (const char* e = std::getenv("RT_PRIM_REBUILD")) opt.rebuild_prim_groups = std::atoi(e) != 0;  // A/B, tests
    return opt;
}
CompileOptions compile_options_for_create(const RtSceneDesc* desc) {
    CompileOptions opt = compile_options_from_env();
    const char* builder = std::getenv("RT_BVH_BUILDER");
    opt.bvh_on_device = desc && (desc->flags & RT_SCENE_BVH_ON_DEVICE) != 0;
    if (builder && !std::strcmp(builder, "device")) opt.bvh_on_device = true;
    if (builder && !std::strcmp(builder, "host")) opt.bvh_on_device = false;
    return opt;
}

// compile_scene with its message in the error channel
static int compile_desc(const RtSceneDesc* desc, CompiledScene* cs, const CompileOptions& opt) {
    std::string err;
    const int st = compile_scene(desc, cs, &err, opt);
    return st != RT_OK ? set_err(st, err) : st;
}

int plan_scene_update(const HeldDesc& held, const CompiledScene& compiled, const RtSceneDesc* desc, UpdatePlan* out) {
    const std::string field = update_mismatch(held.d, *desc);
    if (!field.empty()) return set_err(RT_E_INVALID, update_mismatch_message(field));
    std::vector<bool>&changed = out->changed, &same = out->same;
    changed.assign(desc->n_meshes, false); same.assign(desc->n_meshes, true);
    for (uint32_t i = 0; i < desc->n_meshes; i++) {
        const RtMesh &o = held.meshes[i], &m = desc->meshes[i];
        auto differs = [](const double* x, const double* y, size_t n) { return x && n && std::memcmp(x, y, n * sizeof(double)) != 0; };
        changed[i] = differs(o.positions, m.positions, 3 * size_t(m.n_positions)) || differs(o.normals, m.normals, 3 * size_t(m.n_normals)) ||
                     differs(o.uvs, m.uvs, 3 * size_t(m.n_uvs));
        same[i] = !changed[i];
        if (!changed[i] || !m.positions) continue;
        for (size_t k = 0; k < 3 * size_t(m.n_positions); k++)
            if (!(std::fabs(m.positions[k]) <= 1e37))  // also NaN
                return set_err(RT_E_UNSUPPORTED, "scene update: meshes[" + std::to_string(i) + "].positions: coordinates beyond the f32 grid");
    }
    CompileOptions opt = compile_options_from_env();  // as rt_scene_create
    opt.reuse = &compiled;
    opt.mesh_changed = &changed;
    CompiledScene& cs = out->cs;
    if (int st = compile_desc(desc, &cs, opt)) return st;
    if (cs.mesh_geoms.size() != compiled.mesh_geoms.size() || cs.nodes.size() != compiled.nodes.size() ||
        cs.nodes4.size() != compiled.nodes4.size() || cs.tris.size() != compiled.tris.size())
        return set_err(RT_E_INVALID, update_mismatch_message("mesh tables"));
    out->moved.clear(); out->n_tris_moved = 0;
    for (uint32_t gi = 0; gi < cs.mesh_geoms.size(); gi++)
        if (changed[size_t(cs.mesh_geoms[gi].mesh)]) { out->moved.push_back(gi); out->n_tris_moved += cs.mesh_geoms[gi].n_tris; }
    return RT_OK;
}

// The mesh export from the tables the host derives in arithmetic type R (rt_tables.cpp): what DeviceScene<R>::build uploads
template <typename R>
static int mesh_export_host(const CompiledScene& cs, const CompiledScene::MeshGeom& g, const MeshExportOut& o) {
    MeshTables<R> m;
    std::string err;
    if (int st = derive_mesh_tables(cs, &m, &err)) return set_err(st, err);
    mesh_export<R>(g, m.nodes4qc.data() + g.node4_base, m.tris.data() + g.tri_base, cs.tri_order.data() + g.tri_base, o);
    return RT_OK;
}

// rt_scene_tables_digest for one arithmetic type: the digests of digest_tables() over the derived vectors.
template <typename R>
static int tables_digest_host(const CompiledScene& cs, uint64_t out[8]) {
    MeshTables<R> m;
    SceneTables<R> t;
    std::string err;
    int st;
    if ((st = derive_mesh_tables(cs, &m, &err)) != RT_OK || (st = derive_scene_tables(cs, &t, &err)) != RT_OK) return set_err(st, err);
    const auto tables = digest_tables(cs, m, t);
    for (int k = 0; k < 7; k++) {
        Digest g;
        g.bytes(tables[k].first, tables[k].second);
        out[k] = g.value();
    }
    out[7] = 0;
    return RT_OK;
}

// rt_scene_groups for one arithmetic type: the group tables of derive_scene_tables, the rest from the CompiledScene as
// DeviceScene<R>::build uploads it.
struct GroupExportOut {
    uint32_t* roots; double* group_boxes; uint32_t group_capacity;
    int32_t* children; float* boxes; uint32_t node_capacity;
    int32_t* prims; uint32_t prim_capacity;
    int32_t* guards; uint32_t guard_capacity;
    uint32_t* counts;
};
template <typename R>
static int group_export_host(const CompiledScene& cs, const GroupExportOut& o) {
    SceneTables<R> t;
    std::string err;
    if (int st = derive_scene_tables(cs, &t, &err)) return set_err(st, err);
    o.counts[0] = uint32_t(t.groups.size());
    o.counts[1] = uint32_t(t.group_nodes.size());
    o.counts[2] = uint32_t(cs.group_prims.size());
    o.counts[3] = uint32_t(cs.group_guards.size());
    o.counts[4] = uint32_t(t.view.group_stack_levels);
    o.counts[5] = uint32_t(t.bounds.size());
    for (size_t g = 0; g < t.groups.size() && g < o.group_capacity; g++) {
        if (o.roots) o.roots[g] = t.groups[g].root;
        if (o.group_boxes)
            for (int a = 0; a < 3; a++) { o.group_boxes[6 * g + size_t(a)] = double(t.groups[g].lo[a]); o.group_boxes[6 * g + 3 + size_t(a)] = double(t.groups[g].hi[a]); }
    }
    for (size_t i = 0; i < t.group_nodes.size() && i < o.node_capacity; i++) {
        const BvhNode4q& n = t.group_nodes[i];
        for (int k = 0; k < 4; k++) {
            if (o.children) o.children[4 * i + size_t(k)] = n.child[k];
            if (o.boxes) decode_qbox(n, k, o.boxes + 24 * i + 6 * size_t(k));
        }
    }
    if (o.prims)
        for (size_t j = 0; j < cs.group_prims.size() && j < o.prim_capacity; j++) {
            o.prims[3 * j] = cs.group_prims[j].pc; o.prims[3 * j + 1] = cs.group_prims[j].guard_first; o.prims[3 * j + 2] = cs.group_prims[j].guard_count;
        }
    if (o.guards)
        for (size_t j = 0; j < cs.group_guards.size() && j < o.guard_capacity; j++) o.guards[j] = cs.group_guards[j];
    return RT_OK;
}

int lightmap_select(const RtSceneDesc& d, const CompiledScene& cs, uint32_t node, uint32_t instance, uint32_t width, uint32_t height,
                    const char* who, LmMeshRef* out) {
    const std::string w = std::string(who) + ": ";
    if (width == 0 || width > kLmMaxDim) return set_err(RT_E_INVALID, w + "width must be in 1 .. 16384");
    if (height == 0 || height > kLmMaxDim) return set_err(RT_E_INVALID, w + "height must be in 1 .. 16384");
    if (node >= d.n_nodes) return set_err(RT_E_INVALID, w + "node " + std::to_string(node) + " is out of range");
    const RtNode& n = d.nodes[node];
    if (n.type != RT_NODE_MESH) return set_err(RT_E_INVALID, w + "node " + std::to_string(node) + " is not an RT_NODE_MESH");
    const RtMesh& m = d.meshes[n.mesh];
    if (!m.uvs || !m.tri_uv || m.n_uvs == 0) return set_err(RT_E_UNSUPPORTED, w + "meshes[" + std::to_string(n.mesh) + "] has no uvs / tri_uv: nothing to rasterise");
    std::vector<int32_t> pcs;
    int vol_depth = 0;
    bool in_volume = false;
    for (size_t pc = 0; pc < cs.ops.size(); pc++) {
        const Op& op = cs.ops[pc];
        if (op.type == OP_VOL_BEGIN) vol_depth++;
        if (op.type == OP_VOL_END) vol_depth--;
        if (op.type != OP_MESH || pc >= cs.op_node.size() || cs.op_node[pc] != int32_t(node)) continue;
        if (vol_depth > 0) in_volume = true;
        else pcs.push_back(int32_t(pc));
    }
    if (in_volume) return set_err(RT_E_UNSUPPORTED, w + "node " + std::to_string(node) + " is the boundary of a volume: it has no surface to bake");
    if (instance >= pcs.size())
        return set_err(RT_E_INVALID, w + "instance " + std::to_string(instance) + " is beyond the " + std::to_string(pcs.size()) + " op(s) of node " + std::to_string(node));
    const Op& op = cs.ops[size_t(pcs[instance])];
    const MeshInst& mi = cs.meshes[size_t(op.arg)];
    *out = LmMeshRef{mi.tri_base, mi.n_tris, op.chain, mi.material, int32_t(node), (mi.flags & RT_MESH_FLAT_SHADING) ? 1u : 0u};
    return RT_OK;
}
}  // namespace rt

using namespace rt;
extern "C" {

// Lightmaps (include/rt_mi355.h): the rule of rt_lightmap.h, every triangle x every texel.
int rt_lightmap_texels_desc(const RtSceneDesc* desc, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* hits_out,
                            uint32_t* counts_out) {
    const char* who = "rt_lightmap_texels_desc";
    if (!desc) return set_err(RT_E_INVALID, std::string(who) + ": desc is NULL");
    if (!hits_out) return set_err(RT_E_INVALID, std::string(who) + ": hits_out is NULL");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_from_env())) return st;
    LmMeshRef mesh;
    if (int st = lightmap_select(*desc, cs, node, instance, width, height, who, &mesh)) return st;
    struct Tri { LmUV a, b, c; uint32_t slot; bool live; };
    std::vector<Tri> tris(mesh.n_tris);  // in RtMesh.tri_pos order
    for (uint32_t slot = 0; slot < mesh.n_tris; slot++) {
        const TriAttr<double>& at = cs.attrs[mesh.tri_base + slot];
        tris[cs.tri_order[mesh.tri_base + slot]] = Tri{lm_uv(at.uv0), lm_uv(at.uv1), lm_uv(at.uv2), slot, at.has_uv != 0};
    }
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const LmUV p = {lm_centre(x, width), lm_centre(y, height)};
            const size_t i = size_t(y) * width + x;
            uint32_t count = 0;
            RtRayHit rec = lm_miss_record();
            for (uint32_t t = 0; t < mesh.n_tris; t++) {
                const Tri& tr = tris[t];
                double area, wb, wc;
                if (!tr.live || !lm_covers(tr.a, tr.b, tr.c, p, &area, &wb, &wc)) continue;
                if (count++ == 0) {
                    const size_t s = size_t(mesh.tri_base) + tr.slot;
                    rec = lm_record(cs.tris[s], cs.attrs[s], mesh.flat != 0u, area, wb, wc, cs.chain_offsets.data(), cs.chain_items.data(), cs.xforms.data(),
                                    mesh.chain, mesh.material, mesh.node, int32_t(t));
                }
            }
            hits_out[i] = rec;
            if (counts_out) counts_out[i] = count;
        }
    return RT_OK;
}


const char* rt_last_error(void) { return rt::g_err.c_str(); }

uint32_t rt_owned_rows(uint32_t image_height, const RtRenderParams* params) {
    if (!params) return 0;
    return rt::owned_rows(image_height, params);
}

int rt_scene_update_check(const RtSceneDesc* a, const RtSceneDesc* b) {
    if (!a || !b) return set_err(RT_E_INVALID, "rt_scene_update_check: NULL argument");
    const std::string field = update_mismatch(*a, *b);
    if (!field.empty()) return set_err(RT_E_INVALID, update_mismatch_message(field));
    return RT_OK;
}

int rt_scene_refit_mesh(const RtSceneDesc* a, const RtSceneDesc* b, uint32_t mesh, uint32_t f32, int32_t* children_out, uint32_t* cones_out,
                        float* boxes_out, uint32_t node_capacity, uint32_t* n_nodes_out, double* tris_out, uint32_t* tri_order_out,
                        uint32_t tri_capacity, uint32_t* n_tris_out) {
    if (!a || !b || !n_nodes_out || !n_tris_out) return set_err(RT_E_INVALID, "rt_scene_refit_mesh: NULL argument");
    const std::string field = update_mismatch(*a, *b);
    if (!field.empty()) return set_err(RT_E_INVALID, update_mismatch_message(field));
    CompiledScene ca, cb;
    if (int st = compile_desc(a, &ca, CompileOptions())) return st;
    CompileOptions opt;
    opt.reuse = &ca;  // every mesh refitted, whether it moved or not
    if (int st = compile_desc(b, &cb, opt)) return st;
    const CompiledScene::MeshGeom* g = nullptr;
    if (!mesh_export_range(cb, mesh, &g)) return set_err(RT_E_INVALID, "rt_scene_refit_mesh: mesh index out of range");
    const MeshExportOut o{children_out, cones_out, boxes_out, node_capacity, n_nodes_out, tris_out, tri_order_out, tri_capacity, n_tris_out};
    return f32 ? mesh_export_host<float>(cb, *g, o) : mesh_export_host<double>(cb, *g, o);
}

int rt_scene_tables_digest(const RtSceneDesc* desc, uint32_t f32, uint64_t out[8]) {
    if (!desc || !out) return set_err(RT_E_INVALID, "rt_scene_tables_digest: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_for_create(desc))) return st;  // the device builder runs on the current device
    return f32 ? tables_digest_host<float>(cs, out) : tables_digest_host<double>(cs, out);
}

int rt_scene_info(const RtSceneDesc* desc, uint32_t* flags_out) {
    if (!desc || !flags_out) return set_err(RT_E_INVALID, "rt_scene_info: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, CompileOptions())) return st;
    *flags_out = (cs.zero_weight_stop ? RT_SCENE_INFO_ZERO_WEIGHT_STOP : 0u) | (cs.needs_tex_interpreter ? RT_SCENE_INFO_TEX_INTERPRETER : 0u) |
                 (cs.volumes.empty() ? 0u : RT_SCENE_INFO_VOLUMES);
    return RT_OK;
}

int rt_scene_mesh_stats(const RtSceneDesc* desc, uint64_t out[8]) {
    if (!desc || !out) return set_err(RT_E_INVALID, "rt_scene_mesh_stats: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_from_env())) return st;
    out[0] = cs.tris.size();
    out[1] = cs.nodes.size();
    out[2] = cs.nodes4.size();
    out[3] = cs.max_bvh_depth;
    out[4] = cs.max_bvh4_stack;
    out[5] = cs.ops.size();
    out[6] = cs.n_rebuilt_groups;
    out[7] = cs.n_rebuilt_prims;
    return RT_OK;
}

int rt_debug_handout_replay(const uint32_t* policy, uint32_t n, uint32_t waves, const uint32_t* order, uint32_t n_order, uint32_t* asks_out,
                            uint32_t capacity, uint32_t* n_asks_out, uint32_t* atomics_out) {
    if (!order || !n_asks_out || !atomics_out || (!asks_out && capacity)) return set_err(RT_E_INVALID, "rt_debug_handout_replay: NULL argument");
    if (waves == 0u || waves > 65536u || n_order == 0u) return set_err(RT_E_INVALID, "rt_debug_handout_replay: 1..65536 waves and a non-empty order");
    std::vector<uint8_t> seen(waves, 0);
    for (uint32_t i = 0; i < n_order; i++) {
        if (order[i] >= waves) return set_err(RT_E_INVALID, "rt_debug_handout_replay: wave index out of range");
        seen[order[i]] = 1;
    }
    for (uint32_t g = 0; g < waves; g++)
        if (!seen[g]) return set_err(RT_E_INVALID, "rt_debug_handout_replay: every wave must appear in the order");
    HandoutPolicy hp{2u, kHandoutLeft256, kHandoutLeft128};
    if (policy) hp = HandoutPolicy{policy[0], policy[1], policy[2]};
    // per wave what WaveRange keeps; state 0: before the static range, 1: serving, 2: told "exhausted", 3: ... and asked once more
    struct Wave { uint32_t end = 0; uint8_t state = 0; };
    std::vector<Wave> ws(waves);
    const uint32_t s0 = handout_first(hp, n, waves), start = waves * s0;
    uint32_t cursor = 0, n_asks = 0, open = waves;
    atomics_out[0] = atomics_out[1] = 0;
    auto record = [&](uint32_t g, uint32_t base, uint32_t end) {
        if (n_asks < capacity) { asks_out[3 * size_t(n_asks)] = g; asks_out[3 * size_t(n_asks) + 1] = base; asks_out[3 * size_t(n_asks) + 2] = end; }
        n_asks++;
    };
    for (uint32_t i = 0; open != 0u; i = (i + 1u) % n_order) {
        const uint32_t g = order[i];
        Wave& w = ws[g];
        if (w.state == 3) continue;
        if (w.state == 0) {  // WaveRange::start; an empty static range sends the first fetch on to the cursor, as in wave_fetch
            uint32_t cur = 0;
            handout_static(n, s0, g, &cur, &w.end);
            w.state = 1;
            if (cur < w.end) { record(g, cur, w.end); continue; }
        }
        uint32_t base = 0, end = 0;
        uint32_t& atomics = atomics_out[w.state == 2 ? 1 : 0];
        const bool got = handout_next(hp, n, waves, start, w.end, [&](uint32_t size) { atomics++; const uint32_t old = cursor; cursor += size; return old; }, &base, &end);
        if (got) { w.end = end; record(g, base, end); }
        else record(g, 0xFFFFFFFFu, 0xFFFFFFFFu);
        if (w.state == 2) { w.state = 3; open--; }
        else if (!got) w.state = 2;
    }
    *n_asks_out = n_asks;
    return RT_OK;
}

int rt_scene_mesh_cones(const RtSceneDesc* desc, uint32_t mesh, uint32_t f32, int32_t* children_out, uint32_t* cones_out,
                        uint32_t node_capacity, uint32_t* n_nodes_out, double* tris_out, uint32_t tri_capacity, uint32_t* n_tris_out) {
    if (!desc || !n_nodes_out || !n_tris_out) return set_err(RT_E_INVALID, "rt_scene_mesh_cones: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, CompileOptions())) return st;
    const CompiledScene::MeshGeom* g = nullptr;
    if (!mesh_export_range(cs, mesh, &g)) return set_err(RT_E_INVALID, "rt_scene_mesh_cones: mesh index out of range");
    *n_nodes_out = g->n_nodes4;
    *n_tris_out = g->n_tris;
    if (children_out && cones_out) {
        const MeshExportOut o{children_out, cones_out, nullptr, node_capacity, n_nodes_out, nullptr, nullptr, 0, n_tris_out};
        if (int st = f32 ? mesh_export_host<float>(cs, *g, o) : mesh_export_host<double>(cs, *g, o)) return st;
    }
    if (tris_out)
        for (size_t t = 0; t < g->n_tris && t < tri_capacity; t++) {
            const TriRec<double>& r = cs.tris[g->tri_base + t];
            for (int a = 0; a < 3; a++) { tris_out[9 * t + size_t(a)] = r.v0[a]; tris_out[9 * t + 3 + size_t(a)] = r.e1[a]; tris_out[9 * t + 6 + size_t(a)] = r.e2[a]; }
        }
    return RT_OK;
}

int rt_scene_mesh_slabs(const RtSceneDesc* desc, uint32_t mesh, uint32_t f32, uint32_t* slabs_out, float* bounds_out, float* frames_out,
                        double* pad_out, uint32_t node_capacity, uint32_t* n_nodes_out) {
    if (!desc || !n_nodes_out) return set_err(RT_E_INVALID, "rt_scene_mesh_slabs: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, CompileOptions())) return st;
    const CompiledScene::MeshGeom* g = nullptr;
    if (!mesh_export_range(cs, mesh, &g)) return set_err(RT_E_INVALID, "rt_scene_mesh_slabs: mesh index out of range");
    *n_nodes_out = g->n_nodes4;
    if (pad_out) *pad_out = mesh_pad(cs, *g);
    if (!slabs_out) return RT_OK;
    std::vector<MeshNode4qc> nodes;  // the cone limits are all that depends on the arithmetic type
    std::string err;
    int st;
    if (f32) { MeshTables<float> m; st = derive_mesh_tables(cs, &m, &err); nodes.swap(m.nodes4qc); }
    else { MeshTables<double> m; st = derive_mesh_tables(cs, &m, &err); nodes.swap(m.nodes4qc); }
    if (st != RT_OK) return set_err(st, err);
    for (size_t i = 0; i < g->n_nodes4 && i < node_capacity; i++) {
        const MeshNode4qc& n = nodes[g->node4_base + i];
        for (int k = 0; k < 4; k++) {
            const uint32_t w = n.slabs.word[k];
            slabs_out[4 * i + size_t(k)] = w;
            if (bounds_out) { bounds_out[8 * i + 2 * size_t(k)] = float(int16_t(w & 0xFFFFu)); bounds_out[8 * i + 2 * size_t(k) + 1] = float(int16_t(w >> 16)); }
        }
        if (frames_out) {
            for (int a = 0; a < 3; a++) frames_out[4 * i + size_t(a)] = n.node.org[a];
            frames_out[4 * i + 3] = float(rf_slab_inv_scale(n.node.cell));
        }
    }
    return RT_OK;
}

int rt_scene_program(const RtSceneDesc* desc, int32_t* ops_out, uint32_t capacity, uint32_t* n_ops_out, uint64_t info[8]) {
    if (!desc || !n_ops_out || !info) return set_err(RT_E_INVALID, "rt_scene_program: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_from_env())) return st;
    *n_ops_out = uint32_t(cs.ops.size());
    if (ops_out)
        for (size_t i = 0; i < cs.ops.size() && i < capacity; i++) {
            ops_out[4 * i + 0] = cs.ops[i].type; ops_out[4 * i + 1] = cs.ops[i].arg;
            ops_out[4 * i + 2] = cs.ops[i].skip; ops_out[4 * i + 3] = cs.ops[i].chain;
        }
    const WavefrontPlan plan = plan_wavefront(cs);
    info[0] = cs.mesh_ops.size();
    info[1] = cs.groups.size();
    info[2] = cs.group_nodes4.size();
    info[3] = cs.max_group_stack;
    info[4] = cs.lights.size();
    info[5] = cs.volumes.size();
    info[6] = (plan.split ? 1u : 0u) | (plan.vol_prims ? 2u : 0u) | (plan.multi_mesh ? 4u : 0u) | (plan.groups ? 8u : 0u);
    info[7] = cs.group_prims.size();
    return RT_OK;
}

int rt_scene_groups(const RtSceneDesc* desc, uint32_t f32, uint32_t* roots_out, double* group_boxes_out, uint32_t group_capacity,
                    int32_t* children_out, float* boxes_out, uint32_t node_capacity, int32_t* prims_out, uint32_t prim_capacity,
                    int32_t* guards_out, uint32_t guard_capacity, uint32_t counts_out[6]) {
    if (!desc || !counts_out) return set_err(RT_E_INVALID, "rt_scene_groups: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_from_env())) return st;
    const GroupExportOut o{roots_out, group_boxes_out, group_capacity, children_out, boxes_out, node_capacity, prims_out, prim_capacity,
                           guards_out, guard_capacity, counts_out};
    return f32 ? group_export_host<float>(cs, o) : group_export_host<double>(cs, o);
}

int rt_scene_op_nodes(const RtSceneDesc* desc, int32_t* nodes_out, uint32_t capacity, uint32_t* n_ops_out) {
    if (!desc || !n_ops_out) return set_err(RT_E_INVALID, "rt_scene_op_nodes: NULL argument");
    CompiledScene cs;
    if (int st = compile_desc(desc, &cs, compile_options_from_env())) return st;
    *n_ops_out = uint32_t(cs.op_node.size());
    if (nodes_out)
        for (size_t i = 0; i < cs.op_node.size() && i < capacity; i++) nodes_out[i] = cs.op_node[i];
    return RT_OK;
}

// Light groups (include/rt_mi355.h)
int rt_light_groups_auto(const RtSceneDesc* desc, uint32_t max_groups, int has_background, uint8_t* material_group_out,
                         uint32_t* background_group_out, uint32_t* n_groups_out) {
    if (!desc || !background_group_out || !n_groups_out || (desc->n_materials && !material_group_out))
        return set_err(RT_E_INVALID, "rt_light_groups_auto: NULL argument");
    if (max_groups < 1 || max_groups > RT_LIGHT_GROUPS_MAX) return set_err(RT_E_INVALID, "rt_light_groups_auto: max_groups outside 1 .. RT_LIGHT_GROUPS_MAX");
    if ((desc->n_nodes && !desc->nodes) || (desc->n_child_indices && !desc->child_indices) || (desc->n_materials && !desc->materials))
        return set_err(RT_E_INVALID, "scene description has NULL tables");
    if (desc->world_root >= desc->n_nodes) return set_err(RT_E_INVALID, "world root out of range");
    // materials that a node of `world` references (Sky / Sun: the embedded Emissive), each node visited once
    std::vector<uint8_t> seen(desc->n_nodes, 0), used(desc->n_materials, 0);
    std::vector<uint32_t> todo{desc->world_root};
    seen[desc->world_root] = 1;
    while (!todo.empty()) {
        const RtNode& n = desc->nodes[todo.back()];
        todo.pop_back();
        if (n.material >= 0) {
            if (uint32_t(n.material) >= desc->n_materials) return set_err(RT_E_INVALID, "material index out of range");
            used[n.material] = 1;
        }
        if (n.n_children && uint64_t(n.first_child) + n.n_children > desc->n_child_indices) return set_err(RT_E_INVALID, "child range out of bounds");
        for (uint32_t k = 0; k < n.n_children; k++) {
            const uint32_t c = desc->child_indices[n.first_child + k];
            if (c >= desc->n_nodes) return set_err(RT_E_INVALID, "child index out of range");
            if (!seen[c]) { seen[c] = 1; todo.push_back(c); }
        }
    }
    uint32_t next = 1, highest = 0;
    auto take = [&]() { const uint32_t id = std::min(next++, max_groups - 1u); highest = std::max(highest, id); return id; };
    for (uint32_t m = 0; m < desc->n_materials; m++)
        material_group_out[m] = (used[m] && desc->materials[m].type == RT_MAT_EMISSIVE) ? uint8_t(take()) : uint8_t(0);
    *background_group_out = has_background ? take() : 0u;
    *n_groups_out = highest + 1u;
    return RT_OK;
}

}  // extern "C"
