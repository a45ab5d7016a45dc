// rt_tables.cpp — the kernels' tables from a CompiledScene (rt_tables.h): one function per table or family of tables.
#include "rt_tables.h"

#include <algorithm>
#include <cmath>

#include "rt_refit.h"

namespace rt {

static int refuse(std::string* err, const char* msg) {
    if (err) *err = msg;
    return RT_E_UNSUPPORTED;
}

double mesh_pad(const CompiledScene& cs, const CompiledScene::MeshGeom& g) {
    double pad = 0.0;  // a mesh without nodes shares its base with the next one and has no box: the largest is the mesh's
    for (size_t i = 0; i < cs.meshes.size(); i++)
        if (cs.meshes[i].node4_base == g.node4_base) pad = std::fmax(pad, rf_pad_of_box(cs.mesh_bounds[i].lo, cs.mesh_bounds[i].hi));
    return pad;
}

// ---- the mesh tables ----
template <typename R> static void derive_nodes2(const CompiledScene& cs, std::vector<BvhNode<R>>* out) {
    out->resize(cs.nodes.size());
    for (size_t i = 0; i < out->size(); i++) {
        const BuildNode& s = cs.nodes[i];
        BvhNode<R>& n = (*out)[i];
        // Conservative boxes: outward rounding plus a few ulps so that the slab arithmetic
        // never culls a triangle the exact test would hit.
        for (int a = 0; a < 3; a++) {  // the formula: rt_refit.h
            rf_pad_box2<R>(s.lo0[a], s.hi0[a], &n.lo0[a], &n.hi0[a]);
            rf_pad_box2<R>(s.lo1[a], s.hi1[a], &n.lo1[a], &n.hi1[a]);
        }
        n.c0 = s.c0;
        n.c1 = s.c1;
    }
}

// per mesh node: the pad of its mesh
static std::vector<double> derive_node_pads(const CompiledScene& cs) {
    std::vector<double> pad(cs.nodes4.size(), 0.0);
    for (const CompiledScene::MeshGeom& g : cs.mesh_geoms) std::fill_n(pad.begin() + g.node4_base, g.n_nodes4, mesh_pad(cs, g));
    return pad;
}

// 4-wide f32 nodes: pad by 2^-19 x (largest |coordinate| of the mesh), round outward
static void derive_nodes4f(const CompiledScene& cs, const std::vector<double>& node_pad, std::vector<BvhNode4f>* out) {
    out->resize(cs.nodes4.size());
    for (size_t i = 0; i < out->size(); i++) {
        const BuildNode4& sn = cs.nodes4[i];
        BvhNode4f& dn = (*out)[i];
        for (int k = 0; k < 4; k++) {
            float* lo[3] = {&dn.lox[k], &dn.loy[k], &dn.loz[k]};
            float* hi[3] = {&dn.hix[k], &dn.hiy[k], &dn.hiz[k]};
            for (int a = 0; a < 3; a++) rf_pad_box4f(sn.lo[k][a], sn.hi[k][a], node_pad[i], lo[a], hi[a]);
            dn.child[k] = sn.child[k];
            dn._pad[k] = 0;
        }
    }
}

// one quantised node (the formula: rt_refit.h)
static bool quantise(const BuildNode4& sn, double m, BvhNode4q& qn) {
    for (int k = 0; k < 4; k++) qn.child[k] = sn.child[k];
    return rf_quantise4(sn.lo, sn.hi, sn.child, m, qn.org, qn.cell, qn.qlo, qn.qhi);
}

// Quantised nodes: the padded child boxes (as in BvhNode4f: 2^-19 S, rounded outward to f32) on a per-node 8-bit
// grid, rounded outward on the grid.  k_wf_mesh evaluates t = fma(q, cell * iv, fma(org, iv, -o * iv)): cell is a
// power of two (cell * iv exact), so against the f32-node test (fma(plane, iv, -o * iv)) there is one more rounding,
// of a value bounded by 2 S |iv|; with it the error is < 2.5 x 2^-23 S |iv| per plane, inside the padding.
// With them the back-face cone words of the children, with the conditioning limits of the arithmetic type (rt_bvh.cpp),
// the slab-only axes of inner children without a cone (unless RT_SLAB_AXES=0), and the normal slabs on all those axes.
static int derive_nodes4qc(const CompiledScene& cs, const std::vector<double>& node_pad, bool f32, std::vector<MeshNode4qc>* out, std::string* err) {
    std::vector<BvhNode4q> nodes4q(cs.nodes4.size());
    for (size_t i = 0; i < nodes4q.size(); i++)
        if (!quantise(cs.nodes4[i], node_pad[i], nodes4q[i])) return refuse(err, "BVH node does not fit the 8-bit grid");
    std::vector<uint32_t> cone_words, slab_words;
    build_mesh_cones(cs.nodes4, cs.tris, cone_limits(f32), &cone_words);
    if (slab_axes_enabled()) build_mesh_slab_axes(cs.nodes4, cs.tris, cone_limits(f32), nodes4q.data(), node_pad.data(), &cone_words);
    build_mesh_slabs(cs.nodes4, cs.tris, cone_words, nodes4q.data(), node_pad.data(), &slab_words);
    out->resize(cs.nodes4.size());
    for (size_t i = 0; i < out->size(); i++) {
        MeshNode4qc& n = (*out)[i];
        n.node = nodes4q[i];
        for (int k = 0; k < 4; k++) n.cones.word[k] = cone_words[4 * i + size_t(k)];
        for (int k = 0; k < 4; k++) n.slabs.word[k] = slab_words[4 * i + size_t(k)];
        for (uint32_t& x : n._pad) x = 0;
    }
    return RT_OK;
}

template <typename R> static void derive_triangles(const CompiledScene& cs, std::vector<TriRec<R>>* tris, std::vector<TriAttr<R>>* attrs) {
    tris->resize(cs.tris.size());
    for (size_t i = 0; i < tris->size(); i++) {
        TriRec<R>& t = (*tris)[i];
        cast_arr(t.v0, cs.tris[i].v0); cast_arr(t.e1, cs.tris[i].e1); cast_arr(t.e2, cs.tris[i].e2);
        t._pad = R(0);
    }
    attrs->resize(cs.attrs.size());
    for (size_t i = 0; i < attrs->size(); i++) {
        const auto& s = cs.attrs[i];
        TriAttr<R>& a = (*attrs)[i];
        cast_arr(a.n0, s.n0); cast_arr(a.n1, s.n1); cast_arr(a.n2, s.n2);
        cast_arr(a.uv0, s.uv0); cast_arr(a.uv1, s.uv1); cast_arr(a.uv2, s.uv2);
        a.has_uv = s.has_uv;
        a._pad = 0;
    }
}

template <typename R>
int derive_mesh_tables(const CompiledScene& cs, MeshTables<R>* out, std::string* err) {
    *out = MeshTables<R>{};
    const std::vector<double> node_pad = derive_node_pads(cs);
    derive_nodes2(cs, &out->nodes);
    derive_nodes4f(cs, node_pad, &out->nodes4);
    if (int st = derive_nodes4qc(cs, node_pad, sizeof(R) == 4, &out->nodes4qc, err)) return st;
    derive_triangles(cs, &out->tris, &out->attrs);
    return RT_OK;
}

// ---- the small tables ----
template <typename R> static void derive_prims(const CompiledScene& cs, SceneTables<R>* t) {
    t->bounds.resize(cs.bounds.size());
    for (size_t i = 0; i < t->bounds.size(); i++) {
        // list/bvh bounds are part of the reference's semantics (inverted boxes cull, B-8): nearest rounding
        cast_arr(t->bounds[i].lo, cs.bounds[i].lo);
        cast_arr(t->bounds[i].hi, cs.bounds[i].hi);
    }
    t->xforms.resize(cs.xforms.size());
    for (size_t i = 0; i < t->xforms.size(); i++) {
        cast_arr(t->xforms[i].m, cs.xforms[i].m);
        cast_arr(t->xforms[i].inv, cs.xforms[i].inv);
    }
    t->spheres.resize(cs.spheres.size());
    for (size_t i = 0; i < t->spheres.size(); i++) {
        cast_arr(t->spheres[i].center, cs.spheres[i].center);
        t->spheres[i].radius = R(cs.spheres[i].radius);
        t->spheres[i].material = cs.spheres[i].material;
        t->spheres[i]._pad = 0;
    }
    t->planes.resize(cs.planes.size());
    for (size_t i = 0; i < t->planes.size(); i++) {
        const auto& s = cs.planes[i];
        PlanePrim<R>& p = t->planes[i];
        cast_arr(p.corner, s.corner); cast_arr(p.normal, s.normal);
        cast_arr(p.u, s.u); cast_arr(p.v, s.v);
        cast_arr(p.inv_u, s.inv_u); cast_arr(p.inv_v, s.inv_v);
        p.area = R(s.area);
        p.material = s.material;
        p.backface = s.backface;
    }
    t->suns.resize(cs.suns.size());
    for (size_t i = 0; i < t->suns.size(); i++) {
        cast_arr(t->suns[i].direction, cs.suns[i].direction);
        t->suns[i].material = cs.suns[i].material;
        t->suns[i]._pad = 0;
    }
    t->volumes.resize(cs.volumes.size());
    for (size_t i = 0; i < t->volumes.size(); i++) {
        t->volumes[i].neg_inv_density = R(cs.volumes[i].neg_inv_density);
        t->volumes[i].material = cs.volumes[i].material;
        t->volumes[i]._pad = 0;
    }
}

// the instances' boxes and the records k_wf_mesh enters a mesh op with; after derive_prims (the transforms in R)
template <typename R> static void derive_mesh_ops(const CompiledScene& cs, SceneTables<R>* t) {
    t->mesh_bounds.resize(cs.mesh_bounds.size());
    for (size_t i = 0; i < t->mesh_bounds.size(); i++)
        for (int a = 0; a < 3; a++) {  // outward: this box only decides which rays are queued for the mesh
            t->mesh_bounds[i].lo[a] = round_down<R>(cs.mesh_bounds[i].lo[a]);
            t->mesh_bounds[i].hi[a] = round_up<R>(cs.mesh_bounds[i].hi[a]);
        }
    t->mesh_op_recs.resize(cs.mesh_ops.size());
    for (size_t m = 0; m < t->mesh_op_recs.size(); m++) {
        const Op& op = cs.ops[size_t(cs.mesh_ops[m])];
        const MeshInst& mi = cs.meshes[size_t(op.arg)];
        MeshOpRec<R>& r = t->mesh_op_recs[m];
        r.pc = cs.mesh_ops[m];
        r.chain = op.chain;
        r.node4_base = mi.node4_base;
        const int32_t cb = cs.chain_offsets[size_t(op.chain)], ce = cs.chain_offsets[size_t(op.chain) + 1];
        r.flags = (mi.flags & 0xFFFFu) | (uint32_t(std::min(ce - cb, 0xFFFF)) << 16);
        for (int a = 0; a < 3; a++) { r.lo[a] = t->mesh_bounds[size_t(op.arg)].lo[a]; r.hi[a] = t->mesh_bounds[size_t(op.arg)].hi[a]; }
        for (int k = 0; k < 12; k++) r.inv[k] = ce - cb == 1 ? t->xforms[size_t(cs.chain_items[size_t(cb)])].inv[k] : R(0);
    }
}

// the primitive groups' BVHs: the mesh nodes' format, same padding rule (2^-19 x the largest |coordinate| of the group's box)
template <typename R> static int derive_groups(const CompiledScene& cs, SceneTables<R>* t, std::string* err) {
    t->group_nodes.resize(cs.group_nodes4.size());
    for (size_t g = 0; g < cs.groups.size(); g++) {
        const GroupRec<double>& gr = cs.groups[g];
        double S = 0.0;
        for (int a = 0; a < 3; a++) S = std::fmax(S, std::fmax(std::fabs(gr.lo[a]), std::fabs(gr.hi[a])));
        if (!std::isfinite(S)) return refuse(err, "primitive group with an unbounded box");
        const size_t end = g + 1 < cs.groups.size() ? cs.groups[g + 1].root : cs.group_nodes4.size();
        for (size_t i = gr.root; i < end; i++)
            if (!quantise(cs.group_nodes4[i], S * (1.0 / 524288.0), t->group_nodes[i])) return refuse(err, "group BVH node does not fit the 8-bit grid");
    }
    t->groups.resize(cs.groups.size());
    for (size_t g = 0; g < t->groups.size(); g++) {
        t->groups[g].root = cs.groups[g].root;
        for (int a = 0; a < 3; a++) { t->groups[g].lo[a] = round_down<R>(cs.groups[g].lo[a]); t->groups[g].hi[a] = round_up<R>(cs.groups[g].hi[a]); }
    }
    return RT_OK;
}

template <typename R> static void derive_shading(const CompiledScene& cs, SceneTables<R>* t) {
    t->material_params.resize(cs.material_params.size());
    for (size_t i = 0; i < t->material_params.size(); i++) {
        MaterialParams<R>& p = t->material_params[i];
        p.ior = R(cs.material_params[i].ior);
        p.inv_ior = R(cs.material_params[i].inv_ior);
        auto r0_of = [](R x) { R r0 = (R(1) - x) / (R(1) + x); return r0 * r0; };  // utils.rs:32-33, in R like reflectance()
        p.inv_ior_r = R(1) / p.ior;
        p.r0_glossy = r0_of(p.inv_ior);
        p.r0_front = r0_of(p.inv_ior_r);
        p.r0_back = r0_of(p.ior);
    }
    t->textures.resize(cs.textures.size());
    for (size_t i = 0; i < t->textures.size(); i++) {
        const auto& s = cs.textures[i];
        TextureRec<R>& x = t->textures[i];
        x.type = s.type; x.aux = s.aux; x.data = s.data;
        x.width = s.width; x.height = s.height; x._pad = 0;
        cast_arr(x.v, s.v);
        x.scale = R(s.scale);
    }
    t->perlin_vec.assign(cs.perlin_vec.size(), R(0));
    for (size_t i = 0; i < t->perlin_vec.size(); i++) t->perlin_vec[i] = R(cs.perlin_vec[i]);
}

// the small tables once more, packed for LDS staging: once in k_wf_prims' order, once in k_wf_shade's
template <typename R> static void derive_blobs(const CompiledScene& cs, SceneTables<R>* t) {
    struct Tbl { const void* data; size_t bytes; };
    const Tbl tbl[ST_COUNT] = {
        {cs.ops.data(), cs.ops.size() * sizeof(Op)}, {t->bounds.data(), t->bounds.size() * sizeof(Bounds<R>)},
        {cs.chain_offsets.data(), cs.chain_offsets.size() * 4}, {cs.chain_items.data(), cs.chain_items.size() * 4},
        {t->xforms.data(), t->xforms.size() * sizeof(Xform<R>)}, {t->spheres.data(), t->spheres.size() * sizeof(SpherePrim<R>)},
        {t->planes.data(), t->planes.size() * sizeof(PlanePrim<R>)}, {t->suns.data(), t->suns.size() * sizeof(SunPrim<R>)},
        {cs.meshes.data(), cs.meshes.size() * sizeof(MeshInst)}, {cs.materials.data(), cs.materials.size() * sizeof(MaterialRec)},
        {t->material_params.data(), t->material_params.size() * sizeof(MaterialParams<R>)}, {t->textures.data(), t->textures.size() * sizeof(TextureRec<R>)},
        {cs.lights.data(), cs.lights.size() * sizeof(LightRec)}};
    auto pack = [&](const int (&order)[ST_COUNT], SmallLayout& L, std::vector<char>& blob) {
        for (int k : order) {
            const size_t off = (blob.size() + 15) & ~size_t(15);
            blob.resize(off + tbl[k].bytes);
            if (tbl[k].bytes) std::memcpy(blob.data() + off, tbl[k].data, tbl[k].bytes);
            L.begin[k] = uint32_t(off);
            L.end[k] = uint32_t(off + tbl[k].bytes);
        }
        blob.resize((blob.size() + 15) & ~size_t(15));
        L.total_bytes = uint32_t(blob.size());
    };
    const int order_prims[ST_COUNT] = {ST_OPS, ST_CHAIN_OFFSETS, ST_CHAIN_ITEMS, ST_XFORMS, ST_MESHES, ST_SUNS, ST_PLANES, ST_BOUNDS, ST_SPHERES,
                                       ST_MATERIALS, ST_MATERIAL_PARAMS, ST_LIGHTS, ST_TEXTURES};
    const int order_shade[ST_COUNT] = {ST_OPS, ST_CHAIN_OFFSETS, ST_CHAIN_ITEMS, ST_XFORMS, ST_MESHES, ST_SUNS, ST_LIGHTS, ST_PLANES, ST_MATERIALS,
                                       ST_MATERIAL_PARAMS, ST_TEXTURES, ST_SPHERES, ST_BOUNDS};
    pack(order_prims, t->view.lay, t->blob_prims);
    pack(order_shade, t->view.lay_shade, t->blob_shade);
}

template <typename R>
int derive_scene_tables(const CompiledScene& cs, SceneTables<R>* out, std::string* err) {
    *out = SceneTables<R>{};
    derive_prims(cs, out);
    derive_mesh_ops(cs, out);
    if (int st = derive_groups(cs, out, err)) return st;
    derive_shading(cs, out);
    derive_blobs(cs, out);
    SceneView<R>& v = out->view;
    v.n_mesh_ops = int32_t(cs.mesh_ops.size());
    v.n_group_nodes = int32_t(out->group_nodes.size());
    v.group_stack_levels = int32_t(cs.max_group_stack);
    v.n_lights = cs.n_top_lights;
    v.inv_n_lights = R(1) / R(cs.n_top_lights);
    v.lights_is_list = cs.lights_is_list;
    v.stop_on_zero_weight = cs.zero_weight_stop ? 1 : 0;
    v.stack_entries = int32_t(std::max(cs.max_bvh_depth + 2, cs.max_bvh4_stack + 1));
    v.n_ops = int32_t(cs.ops.size());
    return RT_OK;
}

template int derive_mesh_tables<float>(const CompiledScene&, MeshTables<float>*, std::string*);
template int derive_mesh_tables<double>(const CompiledScene&, MeshTables<double>*, std::string*);
template int derive_scene_tables<float>(const CompiledScene&, SceneTables<float>*, std::string*);
template int derive_scene_tables<double>(const CompiledScene&, SceneTables<double>*, std::string*);

}  // namespace rt
