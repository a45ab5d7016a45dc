// rt_desc.h — the half of the C ABI that works on a description alone (rt_desc.cpp), and what rt_kernels.hip shares with it:
// the description a scene holds, the host half of rt_scene_update, the mesh export.  Plain C++, no HIP.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rt_error.h"
#include "rt_lightmap.h"
#include "rt_tables.h"

namespace rt {

// The description a scene currently holds, as far as rt_scene_update needs it: every structural field, and the meshes'
// arrays (the index arrays belong to the structure, the vertex arrays tell which meshes an update moves).  Texel and noise
// tables are not kept, only whether they are there: they are uploaded again with the small tables at every update.
struct HeldDesc {
    RtSceneDesc d{};
    std::vector<RtNode> nodes;
    std::vector<uint32_t> child_indices;
    std::vector<RtMesh> meshes;
    std::vector<RtMaterial> materials;
    std::vector<RtTexture> textures;
    struct Arrays {
        std::vector<double> positions, normals, uvs;
        std::vector<uint32_t> tri_pos, tri_nrm;
        std::vector<int32_t> tri_uv;
    };
    std::vector<Arrays> arrays;
    void relink() {
        d.nodes = nodes.data(); d.child_indices = child_indices.data(); d.transforms = nullptr; d.meshes = meshes.data();
        d.materials = materials.data(); d.textures = textures.data();
        for (size_t i = 0; i < meshes.size(); i++) {
            RtMesh& m = meshes[i];
            const Arrays& a = arrays[i];
            if (m.positions) m.positions = a.positions.data();
            if (m.normals) m.normals = a.normals.data();
            if (m.uvs) m.uvs = a.uvs.data();
            if (m.tri_pos) m.tri_pos = a.tri_pos.data();
            if (m.tri_nrm) m.tri_nrm = a.tri_nrm.data();
            if (m.tri_uv) m.tri_uv = a.tri_uv.data();
        }
    }
    // a copy of `s` (validated by the compiler); the arrays of mesh i are taken from `old` instead if keep[i]
    void assign(const RtSceneDesc& s, HeldDesc* old = nullptr, const std::vector<bool>* keep = nullptr) {
        static const float kThere = 0.f;
        d = s;
        nodes.assign(s.nodes, s.nodes + s.n_nodes);
        child_indices.assign(s.child_indices, s.child_indices + s.n_child_indices);
        materials.assign(s.materials, s.materials + s.n_materials);
        textures.assign(s.textures, s.textures + s.n_textures);
        for (RtTexture& t : textures) {  // presence only
            if (t.texels) t.texels = &kThere;
            if (t.perlin_vec) t.perlin_vec = reinterpret_cast<const double*>(&kThere);
            if (t.perlin_perm) t.perlin_perm = reinterpret_cast<const uint32_t*>(&kThere);
        }
        std::vector<Arrays> na(s.n_meshes);
        for (uint32_t i = 0; i < s.n_meshes; i++) {
            const RtMesh& m = s.meshes[i];
            if (old && keep && (*keep)[i]) { na[i] = std::move(old->arrays[i]); continue; }
            Arrays& a = na[i];
            if (m.positions) a.positions.assign(m.positions, m.positions + 3 * size_t(m.n_positions));
            if (m.normals) a.normals.assign(m.normals, m.normals + 3 * size_t(m.n_normals));
            if (m.uvs) a.uvs.assign(m.uvs, m.uvs + 3 * size_t(m.n_uvs));
            if (m.tri_pos) a.tri_pos.assign(m.tri_pos, m.tri_pos + 3 * size_t(m.n_triangles));
            if (m.tri_nrm) a.tri_nrm.assign(m.tri_nrm, m.tri_nrm + 3 * size_t(m.n_triangles));
            if (m.tri_uv) a.tri_uv.assign(m.tri_uv, m.tri_uv + 3 * size_t(m.n_triangles));
        }
        meshes.assign(s.meshes, s.meshes + s.n_meshes);
        arrays = std::move(na);
        relink();
    }
};

// Everything an RtSceneDesc points at, field by field (never a pointer value, never padding).  Not the flags: the BVH
// builder only culls, a frame does not depend on it.
uint64_t scene_digest(const RtSceneDesc& d);

// The scene compiler's switches for a scene that is created from `desc`: RT_PRIM_REBUILD, and the BVH builder of the
// description's flag, which RT_BVH_BUILDER = "device" / "host" overrides.
CompileOptions compile_options_for_create(const RtSceneDesc* desc);

// The rows of an image of height h that a render with these params owns (band_rows, n_parts, part).
uint32_t owned_rows(uint32_t h, const RtRenderParams* p);

// The host half of rt_scene_update: everything that can refuse the description, before any device state is touched.
struct UpdatePlan {
    CompiledScene cs;                 // `desc` compiled onto the mesh trees of the scene
    std::vector<bool> changed, same;  // per mesh of the description: its vertex arrays differ from the held ones / do not
    std::vector<uint32_t> moved;      // distinct meshes of the compiled scene whose vertices differ
    uint32_t n_tris_moved = 0;
};
int plan_scene_update(const HeldDesc& held, const CompiledScene& compiled, const RtSceneDesc* desc, UpdatePlan* out);

// Lightmaps (rt_lightmap.h): the argument checks every rasterising entry point shares, host only, and the mesh op that
// (node, instance) names: the instance-th OP_MESH of the compiled program that came from `node`.  RT_OK, or the refusal of
// include/rt_mi355.h with a message that starts with `who` and names the field.
int lightmap_select(const RtSceneDesc& d, const CompiledScene& cs, uint32_t node, uint32_t instance, uint32_t width, uint32_t height,
                    const char* who, LmMeshRef* out);

// Child k's box of a quantised 4-wide node (BvhNode4q), decoded in f32 as the kernels do: lo xyz, hi xyz.
inline void decode_qbox(const BvhNode4q& n, int k, float* out) {
    for (int a = 0; a < 3; a++) {
        out[a] = n.org[a] + float((n.qlo[a] >> (8 * k)) & 255u) * n.cell[a];
        out[3 + a] = n.org[a] + float((n.qhi[a] >> (8 * k)) & 255u) * n.cell[a];
    }
}

// What k_wf_mesh reads of one mesh instance, in the form of rt_scene_refit_mesh / rt_debug_scene_mesh: per node the four
// child references (relative to the mesh), cone words and decoded quantised boxes (org + q cell in f32: lo xyz, hi xyz; an
// empty child has lo > hi), per slot the record widened to double and the original triangle.
struct MeshExportOut {
    int32_t* children; uint32_t* cones; float* boxes; uint32_t node_capacity; uint32_t* n_nodes;
    double* tris; uint32_t* tri_order; uint32_t tri_capacity; uint32_t* n_tris;
};
inline bool mesh_export_range(const CompiledScene& cs, uint32_t mesh, const CompiledScene::MeshGeom** g_out) {
    if (mesh >= cs.meshes.size()) return false;
    for (const CompiledScene::MeshGeom& g : cs.mesh_geoms)
        if (g.node4_base == cs.meshes[mesh].node4_base) { *g_out = &g; return true; }
    return false;
}
template <typename R>
void mesh_export(const CompiledScene::MeshGeom& g, const MeshNode4qc* nodes, const TriRec<R>* tris, const uint32_t* order, const MeshExportOut& o) {
    *o.n_nodes = g.n_nodes4;
    *o.n_tris = g.n_tris;
    for (uint32_t i = 0; i < g.n_nodes4 && i < o.node_capacity; i++) {
        const MeshNode4qc& n = nodes[i];
        for (int k = 0; k < 4; k++) {
            if (o.children) o.children[4 * size_t(i) + size_t(k)] = mesh_relative_child(n.node.child[k], g);
            if (o.cones) o.cones[4 * size_t(i) + size_t(k)] = n.cones.word[k];
            if (o.boxes) decode_qbox(n.node, k, o.boxes + 24 * size_t(i) + 6 * size_t(k));
        }
    }
    for (uint32_t t = 0; t < g.n_tris && t < o.tri_capacity; t++) {
        if (o.tris)
            for (int a = 0; a < 3; a++) {
                o.tris[9 * size_t(t) + size_t(a)] = double(tris[t].v0[a]);
                o.tris[9 * size_t(t) + 3 + size_t(a)] = double(tris[t].e1[a]);
                o.tris[9 * size_t(t) + 6 + size_t(a)] = double(tris[t].e2[a]);
            }
        if (o.tri_order) o.tri_order[t] = order[t];
    }
}

}  // namespace rt
