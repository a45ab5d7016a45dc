// rt_refit.hip — the mesh tables of a scene rewritten ON THE DEVICE for new vertex positions (rt_scene_update).
//
// A mesh keeps its trees (BVH2 and its 4-wide collapse) and its leaf order; only the raw positions / normals / uvs cross
// PCIe.  Per changed mesh and arithmetic type R:
//   1. k_refit_tris<R>   per leaf slot: gather the three vertices through tri_order / tri_pos, write TriRec<R> (edges
//                        subtracted in f64, then rounded) and TriAttr<R>, the exact f64 triangle box and the unit normal
//                        (or the NaN marker of an ill-conditioned triangle, with the limits of R)
//   2. k_refit_up<W>     bottom-up over the BVH2 (W = 2) and the 4-wide tree (W = 4): a node is served by the thread
//                        that finishes the last of its inner children (arrival counter, as k_fit_boxes of
//                        rt_bvh_device.hip).  Exact child boxes are min / max only; the normal sums below a 4-wide child
//                        are added in the host's order (a leaf's triangles in slot order, a node's children in k order)
//                        by ONE thread each: no float atomics, so the sums do not depend on the arrival order.
//   3. k_refit_nodes2<R> / k_refit_nodes4   per node: the reader formats, by the formulas of rt_refit.h that the host
//                        builder uses (BvhNode<R>, BvhNode4f, BvhNode4q, cone and slab words).
//   4. k_refit_slab_axes per inner child without a cone, one block each: the slab-only axis and its slab (unless RT_SLAB_AXES=0).
// The kernels write the fields that depend on the vertices and nothing else: child references and padding keep the bytes
// the host builder gave them, so a refitted table equals, byte for byte, the one DeviceScene<R>::build uploads for the same
// tree and vertices (tests/test_gpu_scene_update.py compares them).
#include "rt_refit.h"

#include <algorithm>

namespace rt {
namespace {

#define REFIT_TRY(expr)                                                                 \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            *err = std::string("scene refit: ") + hipGetErrorString(e_) + " at " #expr; \
            return false;                                                               \
        }                                                                               \
    } while (0)

template <typename R>
__global__ void k_refit_tris(uint32_t n, const uint32_t* __restrict__ tri_order, const uint32_t* __restrict__ tri_pos,
                             const uint32_t* __restrict__ tri_nrm, const int32_t* __restrict__ tri_uv, const double* __restrict__ positions,
                             const double* __restrict__ normals, const double* __restrict__ uvs, ConeLimits lim, TriRec<R>* __restrict__ tris,
                             TriAttr<R>* __restrict__ attrs, double* __restrict__ tri_box, double* __restrict__ tri_normal) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    const size_t t = tri_order[slot];
    const double* p0 = positions + 3 * size_t(tri_pos[3 * t]);
    const double* p1 = positions + 3 * size_t(tri_pos[3 * t + 1]);
    const double* p2 = positions + 3 * size_t(tri_pos[3 * t + 2]);
    double v0[3], e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
        v0[a] = p0[a];
        e1[a] = p1[a] - p0[a];  // mesh.rs:69
        e2[a] = p2[a] - p0[a];  // mesh.rs:70
        tri_box[6 * size_t(slot) + a] = rf_min(p0[a], rf_min(p1[a], p2[a]));
        tri_box[6 * size_t(slot) + 3 + a] = rf_max(p0[a], rf_max(p1[a], p2[a]));
    }
    TriRec<R>& r = tris[slot];
    for (int a = 0; a < 3; a++) { r.v0[a] = R(v0[a]); r.e1[a] = R(e1[a]); r.e2[a] = R(e2[a]); }
    rf_tri_normal(v0, e1, e2, lim, tri_normal + 3 * size_t(slot));
    TriAttr<R>& at = attrs[slot];
    const double* n0 = normals + 3 * size_t(tri_nrm[3 * t]);
    const double* n1 = normals + 3 * size_t(tri_nrm[3 * t + 1]);
    const double* n2 = normals + 3 * size_t(tri_nrm[3 * t + 2]);
    for (int a = 0; a < 3; a++) { at.n0[a] = R(n0[a]); at.n1[a] = R(n1[a]); at.n2[a] = R(n2[a]); }
    const bool has_uv = tri_uv && tri_uv[3 * t] >= 0 && tri_uv[3 * t + 1] >= 0 && tri_uv[3 * t + 2] >= 0;
    if (has_uv) {  // without uvs the record keeps its zeros
        const double* a0 = uvs + 3 * size_t(tri_uv[3 * t]);
        const double* a1 = uvs + 3 * size_t(tri_uv[3 * t + 1]);
        const double* a2 = uvs + 3 * size_t(tri_uv[3 * t + 2]);
        at.uv0[0] = R(a0[0]); at.uv0[1] = R(a0[1]);
        at.uv1[0] = R(a1[0]); at.uv1[1] = R(a1[1]);
        at.uv2[0] = R(a2[0]); at.uv2[1] = R(a2[1]);
    }
}

// parent[] and the number of inner children of every node (once per mesh)
template <int W>
__global__ void k_refit_parents(uint32_t n_nodes, const int32_t* __restrict__ child, int32_t* __restrict__ parent, uint32_t* __restrict__ inner) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    uint32_t cnt = 0;
    for (int k = 0; k < W; k++) {
        const int32_t c = child[W * size_t(i) + k];
        if (c >= 0 && uint32_t(c) < n_nodes) { parent[c] = int32_t(i); cnt++; }
    }
    inner[i] = cnt;
    if (i == 0) parent[0] = -1;
}

// One node: the exact boxes of its W children (and, W = 4, what lies below each: run of slots, count, sum of normals).
template <int W>
__device__ inline void refit_node(uint32_t i, uint32_t n_nodes, uint32_t n_tris, const int32_t* __restrict__ child, const double* __restrict__ tri_box,
                                  const double* __restrict__ tri_normal, double* box, double* sum, uint32_t* run) {
    for (int k = 0; k < W; k++) {
        const int32_t c = child[W * size_t(i) + k];
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double s[3] = {0.0, 0.0, 0.0};
        uint32_t rlo = UINT32_MAX, rhi = 0, cnt = 0;
        if (c != kEmptyChild && c < 0) {
            const uint32_t code = uint32_t(~c), first = code >> 3, count = (code & 7u) + 1u;
            if (first + count <= n_tris) {
                rlo = first; rhi = first + count; cnt = count;
                for (uint32_t t = first; t < first + count; t++) {
                    for (int a = 0; a < 3; a++) {
                        lo[a] = rf_min(lo[a], tri_box[6 * size_t(t) + a]);
                        hi[a] = rf_max(hi[a], tri_box[6 * size_t(t) + 3 + a]);
                        if (W == 4) s[a] += tri_normal[3 * size_t(t) + a];
                    }
                }
            }
        } else if (c != kEmptyChild && uint32_t(c) < n_nodes) {
            // the child's own entries were written before its thread's fence: read them through the L2 (volatile)
            const volatile double* cb = box + 6 * W * size_t(c);
            const volatile double* cs = sum + 3 * W * size_t(c);
            const volatile uint32_t* cr = run + 3 * W * size_t(c);
            for (int j = 0; j < W; j++) {
                if (child[W * size_t(c) + j] == kEmptyChild) continue;
                for (int a = 0; a < 3; a++) {
                    lo[a] = rf_min(lo[a], cb[6 * j + a]);
                    hi[a] = rf_max(hi[a], cb[6 * j + 3 + a]);
                }
                if (W == 4) {
                    rlo = min(rlo, cr[3 * j]); rhi = max(rhi, cr[3 * j + 1]); cnt += cr[3 * j + 2];
                    for (int a = 0; a < 3; a++) s[a] += cs[3 * j + a];
                }
            }
        }
        for (int a = 0; a < 3; a++) {
            box[6 * (W * size_t(i) + k) + a] = lo[a];
            box[6 * (W * size_t(i) + k) + 3 + a] = hi[a];
        }
        if (W == 4) {
            for (int a = 0; a < 3; a++) sum[3 * (W * size_t(i) + k) + a] = s[a];
            run[3 * (W * size_t(i) + k)] = rlo; run[3 * (W * size_t(i) + k) + 1] = rhi; run[3 * (W * size_t(i) + k) + 2] = cnt;
        }
    }
}

template <int W>
__global__ void k_refit_up(uint32_t n_nodes, uint32_t n_tris, const int32_t* __restrict__ child, const int32_t* __restrict__ parent,
                           const uint32_t* __restrict__ inner, unsigned int* __restrict__ arrived, const double* __restrict__ tri_box,
                           const double* __restrict__ tri_normal, double* box, double* sum, uint32_t* run) {
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x;
    if (first >= n_nodes || inner[first] != 0u) return;  // nodes above inner nodes are served by the last child to arrive
    int32_t node = int32_t(first);
    for (uint32_t guard = 0; guard <= n_nodes; guard++) {  // a path to the root has at most n_nodes nodes
        refit_node<W>(uint32_t(node), n_nodes, n_tris, child, tri_box, tri_normal, box, sum, run);
        __threadfence();
        const int32_t up = parent[node];
        if (up < 0 || uint32_t(up) >= n_nodes) return;
        if (atomicAdd(&arrived[up], 1u) + 1u < inner[up]) return;  // a sibling subtree is not finished: its thread will continue
        __threadfence();
        node = up;
    }
}

template <typename R>
__global__ void k_refit_nodes2(uint32_t n_nodes, const double* __restrict__ box, BvhNode<R>* __restrict__ nodes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    BvhNode<R>& n = nodes[i];
    const double* b0 = box + 12 * size_t(i);
    const double* b1 = b0 + 6;
    for (int a = 0; a < 3; a++) {
        rf_pad_box2<R>(b0[a], b0[3 + a], &n.lo0[a], &n.hi0[a]);
        rf_pad_box2<R>(b1[a], b1[3 + a], &n.lo1[a], &n.hi1[a]);
    }
}

__global__ void k_refit_nodes4(uint32_t n_nodes, double pad, const int32_t* __restrict__ child, const double* __restrict__ box,
                               const double* __restrict__ sum, const uint32_t* __restrict__ run, const double* __restrict__ tri_normal,
                               const uint32_t* __restrict__ tri_order, const uint32_t* __restrict__ tri_pos, const double* __restrict__ positions,
                               BvhNode4f* __restrict__ nodes4, MeshNode4qc* __restrict__ nodes4q) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    double lo[4][3], hi[4][3];
    int32_t ch[4];
    for (int k = 0; k < 4; k++) {
        ch[k] = child[4 * size_t(i) + k];
        for (int a = 0; a < 3; a++) { lo[k][a] = box[6 * (4 * size_t(i) + k) + a]; hi[k][a] = box[6 * (4 * size_t(i) + k) + 3 + a]; }
    }
    BvhNode4f& f = nodes4[i];
    for (int k = 0; k < 4; k++) {
        rf_pad_box4f(lo[k][0], hi[k][0], pad, &f.lox[k], &f.hix[k]);
        rf_pad_box4f(lo[k][1], hi[k][1], pad, &f.loy[k], &f.hiy[k]);
        rf_pad_box4f(lo[k][2], hi[k][2], pad, &f.loz[k], &f.hiz[k]);
    }
    float org[3] = {0.f, 0.f, 0.f}, cell[3] = {0.f, 0.f, 0.f};  // a node off the grid: no slabs
    uint32_t qlo[3], qhi[3];
    MeshNode4qc& q = nodes4q[i];
    if (rf_quantise4(lo, hi, ch, pad, org, cell, qlo, qhi))  // never false: the host has checked the coordinates
        for (int a = 0; a < 3; a++) { q.node.org[a] = org[a]; q.node.cell[a] = cell[a]; q.node.qlo[a] = qlo[a]; q.node.qhi[a] = qhi[a]; }
    for (int k = 0; k < 4; k++) {
        uint32_t word = kNeutralCone;
        if (ch[k] != kEmptyChild) {
            const uint32_t* r = run + 3 * (4 * size_t(i) + k);
            word = rf_cone_word(tri_normal, r[0], r[1], r[2], sum + 3 * (4 * size_t(i) + k));
        }
        q.cones.word[k] = word;
        // the slab over the same run of slots: the corners as k_refit_tris forms the records (v0, p1 - p0, p2 - p0 in f64)
        uint32_t slab = kNeutralSlab;
        if (word != kNeutralCone) {
            const uint32_t* r = run + 3 * (4 * size_t(i) + k);
            slab = rf_slab_word(word, org, cell, pad, r[0], r[1], r[2], [&](uint32_t slot, double* v) {
                const size_t t = tri_order[slot];
                const double* p0 = positions + 3 * size_t(tri_pos[3 * t]);
                const double* p1 = positions + 3 * size_t(tri_pos[3 * t + 1]);
                const double* p2 = positions + 3 * size_t(tri_pos[3 * t + 2]);
                for (int a = 0; a < 3; a++) { v[a] = p0[a]; v[3 + a] = p1[a] - p0[a]; v[6 + a] = p2[a] - p0[a]; }
            });
        }
        q.slabs.word[k] = slab;
    }
}

// Slab-only axes (rt_bvh.cpp build_mesh_slab_axes), after k_refit_nodes4: ONE BLOCK per (node, child); the blocks of children
// that are not eligible leave at once.  The block reduces, over the child's whole run of slots, the supports of the candidate
// axes kAxisGroup at a time (minima and maxima: the order of the reduction cannot show), thread 0 picks by the host's rule, and
// a second reduction gives the exact interval of P on the chosen axis, finished by rf_slab_finish as rf_slab_word does.
constexpr int kAxisGroup = 8;
constexpr int kAxisBlock = 256;
constexpr int kAxisWaves = kAxisBlock / 64;

__device__ inline double wave_min(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = rf_min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = rf_max(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(kAxisBlock) void k_refit_slab_axes(uint32_t n_nodes, double pad, const int32_t* __restrict__ child, const double* __restrict__ box,
                                                                const double* __restrict__ sum, const uint32_t* __restrict__ run,
                                                                const uint32_t* __restrict__ tri_order, const uint32_t* __restrict__ tri_pos,
                                                                const double* __restrict__ positions, MeshNode4qc* __restrict__ nodes4q) {
    const size_t id = blockIdx.x;  // 4 x node + child
    const size_t i = id >> 2;
    const int k = int(id & 3u);
    if (i >= n_nodes) return;
    const uint32_t lo = run[3 * id], hi = run[3 * id + 1], count = run[3 * id + 2];
    if (!rf_slab_axis_eligible(child[id], n_nodes, nodes4q[i].cones.word[k], lo, hi, count, sum + 3 * id)) return;  // the whole block
    __shared__ double s_lo[kAxisWaves][kSlabAxes], s_hi[kAxisWaves][kSlabAxes];
    __shared__ double s_p[kAxisWaves][2];
    __shared__ int s_pick;
    const int tid = int(threadIdx.x), wave = tid >> 6, lane = tid & 63;
    auto corners = [&](uint32_t slot, double* v) {  // as k_refit_tris forms the records
        const size_t t = tri_order[slot];
        const double* p0 = positions + 3 * size_t(tri_pos[3 * t]);
        const double* p1 = positions + 3 * size_t(tri_pos[3 * t + 1]);
        const double* p2 = positions + 3 * size_t(tri_pos[3 * t + 2]);
        for (int a = 0; a < 3; a++) { v[a] = p0[a]; v[3 + a] = p1[a] - p0[a]; v[6 + a] = p2[a] - p0[a]; }
    };
    for (int g = 0; g < kSlabAxes; g += kAxisGroup) {
        int q[kAxisGroup][3];
        double mn[kAxisGroup], mx[kAxisGroup];
#pragma unroll
        for (int c = 0; c < kAxisGroup; c++) {
            rf_slab_axis(g + c < kSlabAxes ? g + c : kSlabAxes - 1, q[c]);
            mn[c] = INFINITY;
            mx[c] = -INFINITY;
        }
        for (uint32_t slot = lo + uint32_t(tid); slot < hi; slot += uint32_t(kAxisBlock)) {
            double v[9];
            corners(slot, v);
            for (int c3 = 0; c3 < 3; c3++) {
                double x[3];
                rf_tri_corner(v, c3, x);
#pragma unroll
                for (int c = 0; c < kAxisGroup; c++) {
                    const double p = rf_axis_project(q[c], x);
                    mn[c] = rf_min(mn[c], p);
                    mx[c] = rf_max(mx[c], p);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kAxisGroup; c++) {
            const double a = wave_min(mn[c]), b = wave_max(mx[c]);
            if (lane == 0 && g + c < kSlabAxes) { s_lo[wave][g + c] = a; s_hi[wave][g + c] = b; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double smin[kSlabAxes], smax[kSlabAxes];
        for (int c = 0; c < kSlabAxes; c++) {
            smin[c] = s_lo[0][c];
            smax[c] = s_hi[0][c];
            for (int w = 1; w < kAxisWaves; w++) { smin[c] = rf_min(smin[c], s_lo[w][c]); smax[c] = rf_max(smax[c], s_hi[w][c]); }
        }
        s_pick = rf_slab_axis_pick(box + 6 * id, box + 6 * id + 3, smin, smax);
    }
    __syncthreads();
    const int pick = s_pick;
    if (pick < 0) return;
    const uint32_t word = rf_slab_axis_word(pick);
    int q[3];
    rf_cone_axis(word, q);
    float org[3], cell[3];
    for (int a = 0; a < 3; a++) { org[a] = nodes4q[i].node.org[a]; cell[a] = nodes4q[i].node.cell[a]; }
    const double inv_s = rf_slab_inv_scale(cell);
    if (!(inv_s > 0.0) || !std::isfinite(inv_s) || !std::isfinite(pad)) return;  // rf_slab_word: no slab, so no axis
    double plo = INFINITY, phi = -INFINITY;
    for (uint32_t slot = lo + uint32_t(tid); slot < hi; slot += uint32_t(kAxisBlock)) {
        double v[9];
        corners(slot, v);
        for (int c3 = 0; c3 < 3; c3++) {
            double x[3];
            rf_tri_corner(v, c3, x);
            const double p = rf_slab_project(q, org, inv_s, x);
            plo = rf_min(plo, p);
            phi = rf_max(phi, p);
        }
    }
    plo = wave_min(plo);
    phi = wave_max(phi);
    if (lane == 0) { s_p[wave][0] = plo; s_p[wave][1] = phi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kAxisWaves; w++) { plo = rf_min(plo, s_p[w][0]); phi = rf_max(phi, s_p[w][1]); }
        const uint32_t slab = rf_slab_finish(q, pad, inv_s, plo, phi);
        if (slab != kNeutralSlab) {
            nodes4q[i].cones.word[k] = word;
            nodes4q[i].slabs.word[k] = slab;
        }
    }
}

template <typename T>
bool dev_alloc(DevBuf<T>& p, size_t n, std::string* err) {
    if (p.reserve(std::max<size_t>(n, 1) * sizeof(T)) == RT_OK) return true;
    *err = "scene refit: " + g_err;
    return false;
}
template <typename T>
bool dev_put(DevBuf<T>& dst, const T* src, size_t n, hipStream_t stream, uint64_t* bytes, std::string* err) {
    if (n) REFIT_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
    *bytes += n * sizeof(T);
    return true;
}

inline dim3 grid_for(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

bool refit_mesh_upload(RefitMesh& rm, const RtMesh& m, const uint32_t* tri_order, const int32_t* child2, uint32_t n_nodes, const int32_t* child4,
                       uint32_t n_nodes4, hipStream_t stream, uint64_t* bytes, std::string* err) {
    if (!rm.tri_order) {  // first update of this mesh
        RefitMesh r;
        r.n_tris = m.n_triangles; r.n_nodes = n_nodes; r.n_nodes4 = n_nodes4;
        r.n_positions = m.n_positions; r.n_normals = m.n_normals; r.n_uvs = m.uvs && m.tri_uv ? m.n_uvs : 0;
        const size_t nt = r.n_tris;
        bool ok = dev_alloc(r.tri_order, nt, err) && dev_alloc(r.tri_pos, 3 * nt, err) && dev_alloc(r.tri_nrm, 3 * nt, err) &&
                  (!m.tri_uv || dev_alloc(r.tri_uv, 3 * nt, err)) && dev_alloc(r.child2, 2 * size_t(n_nodes), err) &&
                  dev_alloc(r.child4, 4 * size_t(n_nodes4), err) && dev_alloc(r.parent2, n_nodes, err) && dev_alloc(r.parent4, n_nodes4, err) &&
                  dev_alloc(r.inner2, n_nodes, err) && dev_alloc(r.inner4, n_nodes4, err) && dev_alloc(r.arrived2, n_nodes, err) &&
                  dev_alloc(r.arrived4, n_nodes4, err) && dev_alloc(r.positions, 3 * size_t(r.n_positions), err) &&
                  dev_alloc(r.normals, 3 * size_t(r.n_normals), err) && (!r.n_uvs || dev_alloc(r.uvs, 3 * size_t(r.n_uvs), err)) &&
                  dev_alloc(r.tri_box, 6 * nt, err) && dev_alloc(r.tri_normal, 3 * nt, err) && dev_alloc(r.box2, 12 * size_t(n_nodes), err) &&
                  dev_alloc(r.box4, 24 * size_t(n_nodes4), err) && dev_alloc(r.sum4, 12 * size_t(n_nodes4), err) &&
                  dev_alloc(r.run4, 12 * size_t(n_nodes4), err);
        ok = ok && dev_put(r.tri_order, tri_order, nt, stream, bytes, err) && dev_put(r.tri_pos, m.tri_pos, 3 * nt, stream, bytes, err) &&
             dev_put(r.tri_nrm, m.tri_nrm, 3 * nt, stream, bytes, err) && (!m.tri_uv || dev_put(r.tri_uv, m.tri_uv, 3 * nt, stream, bytes, err)) &&
             dev_put(r.child2, child2, 2 * size_t(n_nodes), stream, bytes, err) && dev_put(r.child4, child4, 4 * size_t(n_nodes4), stream, bytes, err);
        if (!ok) return false;
        // the source arrays of the copies above are the caller's temporaries: finish before returning
        hipLaunchKernelGGL(k_refit_parents<2>, grid_for(n_nodes), dim3(256), 0, stream, n_nodes, r.child2.get(), r.parent2.get(), r.inner2.get());
        hipLaunchKernelGGL(k_refit_parents<4>, grid_for(n_nodes4), dim3(256), 0, stream, n_nodes4, r.child4.get(), r.parent4.get(), r.inner4.get());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { *err = std::string("scene refit: ") + hipGetErrorString(e); return false; }
        rm = std::move(r);
    }
    if (rm.n_tris != m.n_triangles || rm.n_positions != m.n_positions || rm.n_normals != m.n_normals || rm.n_nodes != n_nodes || rm.n_nodes4 != n_nodes4) {
        *err = "scene refit: the mesh has another structure than at its first update";
        return false;
    }
    return dev_put(rm.positions, m.positions, 3 * size_t(rm.n_positions), stream, bytes, err) &&
           dev_put(rm.normals, m.normals, 3 * size_t(rm.n_normals), stream, bytes, err) &&
           (!rm.n_uvs || dev_put(rm.uvs, m.uvs, 3 * size_t(rm.n_uvs), stream, bytes, err));
}

template <typename R>
bool refit_mesh_launch(RefitMesh& rm, const RefitTarget<R>& t, hipStream_t stream, std::string* err) {
    if (rm.n_tris == 0) return true;
    const dim3 block(256);
    REFIT_TRY(hipMemsetAsync(rm.arrived2, 0, size_t(rm.n_nodes) * sizeof(uint32_t), stream));
    REFIT_TRY(hipMemsetAsync(rm.arrived4, 0, size_t(rm.n_nodes4) * sizeof(uint32_t), stream));
    hipLaunchKernelGGL((k_refit_tris<R>), grid_for(rm.n_tris), block, 0, stream, rm.n_tris, rm.tri_order.get(), rm.tri_pos.get(), rm.tri_nrm.get(), rm.uvs ? rm.tri_uv.get() : nullptr,
                       rm.positions.get(), rm.normals.get(), rm.uvs.get(), cone_limits(sizeof(R) == 4), t.tris, t.attrs, rm.tri_box.get(), rm.tri_normal.get());
    hipLaunchKernelGGL((k_refit_up<2>), grid_for(rm.n_nodes), block, 0, stream, rm.n_nodes, rm.n_tris, rm.child2.get(), rm.parent2.get(), rm.inner2.get(), rm.arrived2.get(),
                       rm.tri_box.get(), rm.tri_normal.get(), rm.box2.get(), static_cast<double*>(nullptr), static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL((k_refit_up<4>), grid_for(rm.n_nodes4), block, 0, stream, rm.n_nodes4, rm.n_tris, rm.child4.get(), rm.parent4.get(), rm.inner4.get(), rm.arrived4.get(),
                       rm.tri_box.get(), rm.tri_normal.get(), rm.box4.get(), rm.sum4.get(), rm.run4.get());
    hipLaunchKernelGGL((k_refit_nodes2<R>), grid_for(rm.n_nodes), block, 0, stream, rm.n_nodes, rm.box2.get(), t.nodes);
    hipLaunchKernelGGL(k_refit_nodes4, grid_for(rm.n_nodes4), block, 0, stream, rm.n_nodes4, t.pad4, rm.child4.get(), rm.box4.get(), rm.sum4.get(), rm.run4.get(),
                       rm.tri_normal.get(), rm.tri_order.get(), rm.tri_pos.get(), rm.positions.get(), t.nodes4, t.nodes4q);
    if (slab_axes_enabled() && rm.n_nodes4 > 0)
        hipLaunchKernelGGL(k_refit_slab_axes, dim3(4u * rm.n_nodes4), dim3(kAxisBlock), 0, stream, rm.n_nodes4, t.pad4, rm.child4.get(), rm.box4.get(), rm.sum4.get(),
                           rm.run4.get(), rm.tri_order.get(), rm.tri_pos.get(), rm.positions.get(), t.nodes4q);
    REFIT_TRY(hipGetLastError());
    return true;
}
template bool refit_mesh_launch<float>(RefitMesh&, const RefitTarget<float>&, hipStream_t, std::string*);
template bool refit_mesh_launch<double>(RefitMesh&, const RefitTarget<double>&, hipStream_t, std::string*);

}  // namespace rt
