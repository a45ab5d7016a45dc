// rt_tables.h — every table the kernels read, derived from a CompiledScene on the host (plain C++, no HIP).
//
// DeviceScene<R>::build (rt_kernels.hip) uploads these vectors as they stand; the host exports of rt_desc.cpp
// (rt_scene_refit_mesh, rt_scene_mesh_cones, rt_scene_mesh_slabs, rt_scene_tables_digest) read the same vectors.  The per-node formulas are
// those of rt_refit.h and rt_bvh.cpp; compiled with -ffp-contract=off like the rest of the library.
#pragma once
#include <array>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rt_compile.h"

namespace rt {

// 64-bit digest of byte strings (checkpoint identity, not security): 8-byte words through a multiply-rotate round
struct Digest {
    uint64_t h = 0x243F6A8885A308D3ull;
    void word(uint64_t w) {
        w *= 0x9E3779B97F4A7C15ull;
        w ^= w >> 29;
        h = ((h ^ w) * 0xBF58476D1CE4E5B9ull);
        h = (h << 27) | (h >> 37);
    }
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        word(n);
        if (!b) return;
        for (; n >= 8; n -= 8, b += 8) { uint64_t w; std::memcpy(&w, b, 8); word(w); }
        if (n) { uint64_t w = 0; std::memcpy(&w, b, n); word(w); }
    }
    template <typename T> void val(const T& v) { bytes(&v, sizeof v); }
    uint64_t value() const { uint64_t x = h ^ (h >> 31); x *= 0x94D049BB133111EBull; return x ^ (x >> 29); }
};

template <typename R, size_t N> void cast_arr(R (&dst)[N], const double (&src)[N]) {
    for (size_t i = 0; i < N; i++) dst[i] = R(src[i]);
}

// A child reference of CompiledScene::nodes4 (absolute) relative to its mesh: inner = node inside the mesh, leaf =
// ~(slot inside the mesh << 3 | count - 1), kEmptyChild as it is.
inline int32_t mesh_relative_child(int32_t child, const CompiledScene::MeshGeom& g) {
    if (child == kEmptyChild) return child;
    if (child >= 0) return child - int32_t(g.node4_base);
    const uint32_t code = uint32_t(~child);
    return ~int32_t((((code >> 3) - g.tri_base) << 3) | (code & 7u));
}

// The pad of the 4-wide nodes of mesh `g`: rf_pad_of_box of the mesh's box, which every instance of the mesh carries.
double mesh_pad(const CompiledScene& cs, const CompiledScene::MeshGeom& g);

// The mesh tables (every distinct mesh of the scene, in CompiledScene's order), as rt_scene_update's kernels rewrite them.
template <typename R>
struct MeshTables {
    std::vector<BvhNode<R>> nodes;
    std::vector<BvhNode4f> nodes4;
    std::vector<MeshNode4qc> nodes4qc;  // quantised nodes with their cone and slab words
    std::vector<TriRec<R>> tris;
    std::vector<TriAttr<R>> attrs;
};

// Everything else a SceneView<R> points at that is not a table of CompiledScene itself.
template <typename R>
struct SceneTables {
    std::vector<Bounds<R>> bounds;
    std::vector<Xform<R>> xforms;
    std::vector<SpherePrim<R>> spheres;
    std::vector<PlanePrim<R>> planes;
    std::vector<SunPrim<R>> suns;
    std::vector<VolumeRec<R>> volumes;
    std::vector<Bounds<R>> mesh_bounds;  // rounded outward
    std::vector<MeshOpRec<R>> mesh_op_recs;
    std::vector<GroupRec<R>> groups;
    std::vector<BvhNode4q> group_nodes;
    std::vector<MaterialParams<R>> material_params;
    std::vector<TextureRec<R>> textures;
    std::vector<R> perlin_vec;
    std::vector<char> blob_prims, blob_shade;  // the small tables packed in k_wf_prims' order and in k_wf_shade's
    SceneView<R> view{};  // the blobs' layouts and the scalar fields; the pointers stay NULL for whoever uploads the tables
};

// RT_OK, or RT_E_UNSUPPORTED with *err set: a node that does not fit the 8-bit grid, a primitive group without bounds.
template <typename R> int derive_mesh_tables(const CompiledScene& cs, MeshTables<R>* out, std::string* err);
template <typename R> int derive_scene_tables(const CompiledScene& cs, SceneTables<R>* out, std::string* err);

// The seven tables of rt_debug_scene_mesh_digest / rt_scene_tables_digest, in their order, as (pointer, bytes): from the
// derived vectors' data() or from a SceneView's device pointers.
template <typename R>
std::array<std::pair<const void*, size_t>, 7> digest_tables(const CompiledScene& cs, const BvhNode<R>* nodes, const BvhNode4f* nodes4,
                                                            const MeshNode4qc* nodes4q, const TriRec<R>* tris, const TriAttr<R>* attrs,
                                                            const Bounds<R>* mesh_bounds, const MeshOpRec<R>* mesh_op_recs) {
    return {{{nodes, cs.nodes.size() * sizeof(BvhNode<R>)},
             {nodes4, cs.nodes4.size() * sizeof(BvhNode4f)},
             {nodes4q, cs.nodes4.size() * sizeof(MeshNode4qc)},
             {tris, cs.tris.size() * sizeof(TriRec<R>)},
             {attrs, cs.attrs.size() * sizeof(TriAttr<R>)},
             {mesh_bounds, cs.mesh_bounds.size() * sizeof(Bounds<R>)},
             {mesh_op_recs, cs.mesh_ops.size() * sizeof(MeshOpRec<R>)}}};
}
template <typename R>
std::array<std::pair<const void*, size_t>, 7> digest_tables(const CompiledScene& cs, const MeshTables<R>& m, const SceneTables<R>& s) {
    return digest_tables<R>(cs, m.nodes.data(), m.nodes4.data(), m.nodes4qc.data(), m.tris.data(), m.attrs.data(), s.mesh_bounds.data(),
                            s.mesh_op_recs.data());
}

}  // namespace rt
