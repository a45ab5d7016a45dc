// rt_bvh.h — host-side binned-SAH BVH2 builder for one triangle mesh.
//
// Replaces the reference's octree (src/object/mesh/octree.rs:31-210: midpoint split into 8
// octants, <= 50 triangles per leaf, triangles duplicated into every octant they touch,
// children visited in fixed order).  Any structure that returns the same closest hit is
// admissible: the octree only culls; ties between different triangles at exactly
// equal t may resolve to a different (adjacent) triangle.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rt_scene.h"

namespace rt {

struct BuildNode {
    double lo0[3], hi0[3], lo1[3], hi1[3];
    int32_t c0, c1;  // encoding: see BvhNode in rt_scene.h
};

struct BvhBuild {
    std::vector<BuildNode> nodes;     // nodes[0] is the root
    std::vector<uint32_t> tri_order;  // leaf order -> original triangle index
    uint32_t max_depth = 0;           // number of inner-node levels (bounds the traversal stack)
};

// positions: n_positions*3 doubles; tri_pos: n_tris*3 indices.  max_leaf in 1..8.
BvhBuild build_bvh(const double* positions, const uint32_t* tri_pos, uint32_t n_tris, uint32_t max_leaf);

// The same contract, built on the current HIP device (rt_bvh_device.hip: Morton codes, radix sort, Karras radix
// tree, bottom-up box fit).  Returns false with `err` set on a device error.
bool build_bvh_device(const double* positions, uint32_t n_positions, const uint32_t* tri_pos, uint32_t n_tris, uint32_t max_leaf,
                      BvhBuild* out, std::string* err);

// W-wide collapse of a BVH2 (same leaves, same triangle order): every node holds up to W children,
// obtained by repeatedly replacing the inner child of largest surface area by its two children.  One node
// fetch then decides W boxes: about half the dependent fetches per ray for W = 4 (W = 8 was tried with quantised
// nodes and was slower: profiles/r02/ab/node_width_and_size.txt).
template <int W>
struct BuildNodeN {
    double lo[W][3], hi[W][3];
    int32_t child[W];  // same encoding as BuildNode::c0 (inner index into the wide node array / leaf code / kEmptyChild)
};
template <int W>
struct BvhNBuild {
    std::vector<BuildNodeN<W>> nodes;  // nodes[0] is the root
    uint32_t max_depth = 0;            // inner levels
    uint32_t max_stack = 0;            // worst-case traversal stack entries (sum over a root-leaf path of children-1) + 1
    double root_lo[3], root_hi[3];
};
using BuildNode4 = BuildNodeN<4>;
using Bvh4Build = BvhNBuild<4>;
Bvh4Build collapse_bvh4(const BvhBuild& bvh2);

// Back-face cones of the 4-wide mesh nodes (k_wf_mesh): one word of four signed bytes (ax, ay, az, w) per child, four
// words per node, in node order.  With the ray's object-space direction packed as (round(127 d / |d|), -127), the integer
// product `dir . cone > 0` proves that every triangle below the child faces away from the ray, so that the
// reference's front-face rule (mesh.rs:77) rejects each of them: the child need not be entered.  kNeutralCone (rt_scene.h)
// never culls.  The argument, with its numbers, stands beside the builder in rt_bvh.cpp.
struct ConeLimits {
    double sigma;     // a triangle is ill-conditioned if |e1 x e2| < sigma |e1| |e2|
    double min_edge;  // ... or if an edge is shorter / longer than this (no under- or overflow in the determinant's products)
    double max_edge;
};
// the limits for triangle tests in f64 (f32 = false) or in f32 on records rounded to f32
ConeLimits cone_limits(bool f32);
// nodes4: 4-wide nodes with ABSOLUTE child / triangle references (CompiledScene::nodes4), children behind their parent;
// tris: the f64 records in leaf order.  out: 4 words per node.
void build_mesh_cones(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const ConeLimits& lim,
                      std::vector<uint32_t>* out);
// Slab-only axes: an inner child that build_mesh_cones left without a cone gets the word (qx, qy, qz, 127), |q|_2 <= 126, of the
// table direction along which the surface below it is thinnest against its box, if that pays (rt_refit.h rf_slab_axis_pick).
// The word never culls as a cone; build_mesh_slabs reads its axis.  Called between the two; cones: in and out.
void build_mesh_slab_axes(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const ConeLimits& lim,
                          const BvhNode4q* qnodes, const double* node_pad, std::vector<uint32_t>* cones);
// The normal slabs of the same children (rt_scene.h NodeSlabs4).  cones: what the two above gave; qnodes: the quantised
// nodes (grid origin and cells); node_pad: per node the pad of its mesh (rf_pad_of_box).  out: 4 words per node.
void build_mesh_slabs(const std::vector<BuildNode4>& nodes4, const std::vector<TriRec<double>>& tris, const std::vector<uint32_t>& cones,
                      const BvhNode4q* qnodes, const double* node_pad, std::vector<uint32_t>* out);

}  // namespace rt
