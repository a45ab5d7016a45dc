// rt_kernels.hip — the megakernel, the wavefront driver and everything that names a wavefront kernel or builds the path pool
// (build_pool, query_search_pass, the table modes), a scene's creation, update and destruction, and the entry points of the
// C ABI (include/rt_mi355.h) of renders, light groups, AOVs and table modes.  Elsewhere: ray queries (rt_query.hip), point
// queries (rt_point.hip), the ambient-occlusion bake (rt_bake.hip) and lightmaps (rt_lightmap.hip), host side and entry
// points beside their kernels, on the RtScene of rt_scene_host.h; the progressive accumulator (rt_accum.hip, a client of
// this file through rt_render.h); the denoiser (rt_aov.hip); what takes a description alone (rt_desc.cpp).
// gfx950 only: 64-lane waves, per-lane traversal stack in LDS, HIP events on the launch stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <variant>
#include <vector>

#include "rt_aov.h"
#include "rt_compile.h"
#include "rt_desc.h"
#include "rt_device.h"
#include "rt_owned.h"
#include "rt_refit.h"
#include "rt_render.h"
#include "rt_scene_host.h"
#include "rt_tables.h"
#include "rt_wavefront.h"

namespace rt {

// ---------------------------------------------------------------------------------------------
// Megakernel: one lane owns one pixel and walks its samples in the reference's order
// (replica tid, then sy, sx: camera.rs:197,217-218), one bounce per loop trip.  A lane whose path
// ended starts its next sample in the same trip, so the wave stays converged on
// world_test -> shade and no lane idles while it still has samples.  Sums are accumulated
// per pixel in the reference's order, so the result does not depend on scheduling.
// One launch renders the replicas [t_first, t_first + n_rep) of the frame; with t_first > 0 the
// pixel's sum starts from the running sum of [0, t_first) that `out` holds (progressive rendering,
// RtAccum), so any split of [0, T) into launches gives the one-launch frame bit for bit.
// ---------------------------------------------------------------------------------------------
template <typename R, bool STATS, bool TEX>
__global__ void __launch_bounds__(256) k_megakernel(SceneView<R> sc, CameraView<R> cam, ParamsView<R> prm,
                                                    double* __restrict__ out, DeviceCounters* counters, uint32_t t_first,
                                                    uint32_t n_rep) {
    extern __shared__ int lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles_x = (cam.width + 15u) / 16u;
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t px = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t row = by * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (px >= cam.width || row >= prm.owned_rows) return;
    const uint32_t py = row_to_y(prm, row);
    int* stack = lds_stack + threadIdx.x;
    const int stride = int(blockDim.x);

    const uint32_t S = cam.sqrt_spt;
    const uint32_t per_replica = S * S;
    const uint32_t total = per_replica * n_rep;
    const uint64_t pixel_index = uint64_t(py) * cam.width + px;
    double* o = out + (size_t(row) * cam.width + px) * 4;

    LaneCounters cnt;
    double acc[3] = {0.0, 0.0, 0.0};  // buf += thread_buf, camera.rs:247-253
    if (t_first > 0)
        for (int k = 0; k < 3; k++) acc[k] = o[k];
    double col[3] = {0.0, 0.0, 0.0};  // `color` of the current replica, camera.rs:215-229
    uint32_t sample = 0;              // next sample to start
    uint32_t in_replica = 0;
    bool alive = false;
    PathState<R> ps;
    Rng rng;
    rng.s = 0;

    for (;;) {
        if (!alive) {
            if (sample == total) break;
            uint32_t tid = sample / per_replica;
            uint32_t st = sample - tid * per_replica;
            tid += t_first;
            uint32_t sy = st / S, sx = st - sy * S;
            rng.key(prm.seed, tid, pixel_index, st);
            ps.ray = get_ray(cam, px, py, sx, sy, rng);
            ps.throughput = mk<R>(1, 1, 1);
            ps.radiance = mk<R>(0, 0, 0);
            ps.depth = cam.max_depth;
            alive = true;
            sample++;
        }
        bool cont = false;
        if (ps.depth != 0) {
            Best<R> best;
            world_test<R, STATS, TEX>(sc, ps.ray, R(0.001), best, stack, stride, cnt, &rng);  // TEX variant = full feature set (+ volumes)
            cont = shade<R, STATS, TEX>(sc, prm, ps, best, rng, cnt);
            ps.depth--;
            if (cont && ps.depth == 0) {  // ray_color(depth == 0) returns black without tracing (camera.rs:290)
                end_black(ps);
                cont = false;
            }
        }
        if (!cont) {
            alive = false;
            col[0] += double(ps.radiance.x);
            col[1] += double(ps.radiance.y);
            col[2] += double(ps.radiance.z);
            if (++in_replica == per_replica) {
                in_replica = 0;
                for (int k = 0; k < 3; k++) {
                    acc[k] += col[k] / prm.spp;  // color /= samples_per_pixel (total), camera.rs:229
                    col[k] = 0.0;
                }
            }
        }
    }
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
    o[3] = 0.0;
    if (STATS) {
        atomicAdd(&counters->rays, (unsigned long long)cnt.rays);
        atomicAdd(&counters->mesh_rays, (unsigned long long)cnt.mesh_rays);
        atomicAdd(&counters->node_visits, (unsigned long long)cnt.node_visits);
        atomicAdd(&counters->tri_tests, (unsigned long long)cnt.tri_tests);
        atomicAdd(&counters->prim_tests, (unsigned long long)cnt.prim_tests);
    }
}

// Diagnostic probe: one sample traced by one lane, with a per-bounce record
// (17 doubles: t, pos xyz, material, op type, triangle slot, 0, normal xyz, ray origin xyz, ray dir xyz).
// Used by the parity tests to localise differences.
template <typename R>
__global__ void k_trace_sample(SceneView<R> sc, CameraView<R> cam, ParamsView<R> prm, uint32_t tid, uint32_t px, uint32_t py,
                               uint32_t sx, uint32_t sy, double* rgb, double* trace, uint32_t max_bounces, uint32_t* n_out) {
    extern __shared__ int lds_stack[];
    if (threadIdx.x != 0) return;
    LaneCounters cnt;
    Rng rng;
    rng.key(prm.seed, tid, uint64_t(py) * cam.width + px, sy * cam.sqrt_spt + sx);
    PathState<R> ps;
    ps.ray = get_ray(cam, px, py, sx, sy, rng);
    ps.throughput = mk<R>(1, 1, 1);
    ps.radiance = mk<R>(0, 0, 0);
    ps.depth = cam.max_depth;
    uint32_t n = 0;
    while (ps.depth != 0) {
        Best<R> best;
        world_test<R, false, true>(sc, ps.ray, R(0.001), best, lds_stack, int(blockDim.x), cnt, &rng);
        if (n < max_bounces) {
            double* t = trace + 17 * n;
            for (int k = 0; k < 17; k++) t[k] = 0;
            t[0] = double(best.t);
            t[4] = -1; t[5] = -1; t[6] = double(best.tri);
            if (best.pc >= 0) {
                HitInfo<R> h = resolve_hit<R, true>(sc, ps.ray, best);
                t[1] = double(h.pos.x); t[2] = double(h.pos.y); t[3] = double(h.pos.z);
                t[4] = double(h.material);
                t[5] = double(sc.ops[best.pc].type);
                t[8] = double(h.normal.x); t[9] = double(h.normal.y); t[10] = double(h.normal.z);
            }
            t[11] = double(ps.ray.o.x); t[12] = double(ps.ray.o.y); t[13] = double(ps.ray.o.z);
            t[14] = double(ps.ray.d.x); t[15] = double(ps.ray.d.y); t[16] = double(ps.ray.d.z);
        }
        n++;
        bool cont = shade<R, false, true>(sc, prm, ps, best, rng, cnt);  // the general (interpreter) texture path
        ps.depth--;
        if (cont && ps.depth == 0) end_black(ps);
        if (!cont) break;
    }
    rgb[0] = double(ps.radiance.x); rgb[1] = double(ps.radiance.y); rgb[2] = double(ps.radiance.z);
    *n_out = n;
}

// Diagnostic probe: ONE path vertex per lane, what one loop trip of k_megakernel does to a path with throughput (1,1,1) and
// radiance 0 - world_test (with the generator: the volumes' free-flight draws), then shade - from a caller-supplied ray and
// generator state.  RT_SHADE_RAYS_STRIDE doubles per ray (include/rt_mi355.h, rt_debug_shade_rays).  The hit is resolved a
// second time for the record; shade() resolves its own.
template <typename R, bool TEX>
__global__ void __launch_bounds__(256) k_shade_rays(SceneView<R> sc, ParamsView<R> prm, uint32_t n, const double* __restrict__ rays,
                                                    const unsigned long long* __restrict__ states, double* __restrict__ out,
                                                    unsigned long long* __restrict__ state_out) {
    extern __shared__ int lds_stack[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * size_t(i);
    double* o = out + RT_SHADE_RAYS_STRIDE * size_t(i);
    for (int k = 0; k < RT_SHADE_RAYS_STRIDE; k++) o[k] = 0.0;
    LaneCounters cnt;
    Rng rng;
    rng.s = states[i];
    PathState<R> ps;
    ps.ray = make_ray(mk<R>(R(r[0]), R(r[1]), R(r[2])), mk<R>(R(r[3]), R(r[4]), R(r[5])));
    ps.throughput = mk<R>(1, 1, 1);
    ps.radiance = mk<R>(0, 0, 0);
    ps.depth = 1;
    Best<R> best;
    world_test<R, false, TEX>(sc, ps.ray, R(0.001), best, lds_stack + threadIdx.x, int(blockDim.x), cnt, &rng);
    o[0] = double(best.t);
    o[10] = -1.0;
    o[11] = -1.0;
    o[26] = double((rng.s - states[i]) * 0xF1DE83E19937733Dull);  // draws of the search: times the inverse of Rng::next's increment
    if (best.pc >= 0) {
        const HitInfo<R> h = resolve_hit<R, TEX>(sc, ps.ray, best);
        o[1] = double(h.pos.x); o[2] = double(h.pos.y); o[3] = double(h.pos.z);
        o[4] = double(h.normal.x); o[5] = double(h.normal.y); o[6] = double(h.normal.z);
        o[7] = double(h.u); o[8] = double(h.v);
        o[9] = h.front_face ? 1.0 : 0.0;
        o[10] = double(h.material);
        o[11] = double(sc.ops[best.pc].type);
        o[12] = double(h.tex_a.x); o[13] = double(h.tex_a.y); o[14] = double(h.tex_a.z);
        o[15] = double(h.tex_b);
    }
    const bool cont = shade<R, false, TEX>(sc, prm, ps, best, rng, cnt);
    if (cont) {
        o[16] = 1.0;
        o[17] = double(ps.ray.d.x); o[18] = double(ps.ray.d.y); o[19] = double(ps.ray.d.z);
    }
    o[20] = double(ps.throughput.x); o[21] = double(ps.throughput.y); o[22] = double(ps.throughput.z);
    o[23] = double(ps.radiance.x); o[24] = double(ps.radiance.y); o[25] = double(ps.radiance.z);
    state_out[i] = rng.s;
}

// ---------------------------------------------------------------------------------------------
// Host side.  RtScene, its tables on the device and its workspaces: rt_scene_host.h.
// ---------------------------------------------------------------------------------------------
template <typename R>
int DeviceScene<R>::build(const CompiledScene& cs, const DeviceScene<R>* keep) {
    MeshTables<R> m;
    SceneTables<R> t;
    std::string err;
    int st;
    if (!keep && (st = derive_mesh_tables(cs, &m, &err)) != RT_OK) return set_err(st, err);
    if ((st = derive_scene_tables(cs, &t, &err)) != RT_OK) return set_err(st, err);
    view = t.view;  // the scalars and the blobs' layouts; then every table into a buffer of its own
    if ((st = buf.upload(cs.ops, &view.ops)) != RT_OK) return st;
    if ((st = buf.upload(t.bounds, &view.bounds)) != RT_OK) return st;
    if ((st = buf.upload(cs.chain_offsets, &view.chain_offsets)) != RT_OK) return st;
    if ((st = buf.upload(cs.chain_items, &view.chain_items)) != RT_OK) return st;
    if ((st = buf.upload(t.xforms, &view.xforms)) != RT_OK) return st;
    if ((st = buf.upload(t.spheres, &view.spheres)) != RT_OK) return st;
    if ((st = buf.upload(t.planes, &view.planes)) != RT_OK) return st;
    if ((st = buf.upload(t.suns, &view.suns)) != RT_OK) return st;
    if ((st = buf.upload(cs.meshes, &view.meshes)) != RT_OK) return st;
    if ((st = buf.upload(t.volumes, &view.volumes)) != RT_OK) return st;
    if (!keep) {
        if ((st = buf.upload(m.nodes, &view.nodes)) != RT_OK) return st;
        if ((st = buf.upload(m.nodes4, &view.nodes4)) != RT_OK) return st;
        if ((st = buf.upload(m.nodes4qc, &view.nodes4q)) != RT_OK) return st;
        if ((st = buf.upload(m.tris, &view.tris)) != RT_OK) return st;
        if ((st = buf.upload(m.attrs, &view.attrs)) != RT_OK) return st;
    } else {
        view.nodes = keep->view.nodes; view.nodes4 = keep->view.nodes4; view.nodes4q = keep->view.nodes4q;
        view.tris = keep->view.tris; view.attrs = keep->view.attrs;
    }
    if ((st = buf.upload(t.mesh_bounds, &view.mesh_bounds)) != RT_OK) return st;
    if ((st = buf.upload(cs.mesh_ops, &view.mesh_ops)) != RT_OK) return st;
    if ((st = buf.upload(t.mesh_op_recs, &view.mesh_op_recs)) != RT_OK) return st;
    if ((st = buf.upload(t.groups, &view.groups)) != RT_OK) return st;
    if ((st = buf.upload(t.group_nodes, &view.group_nodes)) != RT_OK) return st;
    if ((st = buf.upload(cs.group_prims, &view.group_prims)) != RT_OK) return st;
    if ((st = buf.upload(cs.group_guards, &view.group_guards)) != RT_OK) return st;
    if ((st = buf.upload(cs.materials, &view.materials)) != RT_OK) return st;
    if ((st = buf.upload(t.material_params, &view.material_params)) != RT_OK) return st;
    if ((st = buf.upload(t.textures, &view.textures)) != RT_OK) return st;
    if ((st = buf.upload(cs.texels, &view.texels)) != RT_OK) return st;
    if ((st = buf.upload(t.perlin_vec, &view.perlin_vec)) != RT_OK) return st;
    if ((st = buf.upload(cs.perlin_perm, &view.perlin_perm)) != RT_OK) return st;
    if ((st = buf.upload(cs.lights, &view.lights)) != RT_OK) return st;
    if ((st = buf.upload(t.blob_prims, &view.small_blob)) != RT_OK) return st;
    if ((st = buf.upload(t.blob_shade, &view.small_blob_shade)) != RT_OK) return st;
    if (const char* e = std::getenv("RT_ZERO_WEIGHT_STOP")) view.stop_on_zero_weight = std::atoi(e) != 0;  // experiments
    // The uploads above went through the null stream (small pageable copies may return once
    // staged); the render kernels run on a NON-BLOCKING stream that is not ordered against it.
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}
template <typename R>
void DeviceScene<R>::take_mesh_tables(DeviceScene<R>& from) {
    for (const void* p : {(const void*)view.nodes, (const void*)view.nodes4, (const void*)view.nodes4q, (const void*)view.tris, (const void*)view.attrs})
        buf.adopt(from.buf, p);
}
template struct DeviceScene<float>;
template struct DeviceScene<double>;

template <typename R> CameraView<R> make_camera_view(const RtCameraDesc& c, const RtRenderParams& p) {
    CameraView<R> v{};
    for (int i = 0; i < 3; i++) {
        v.position[i] = R(c.position[i]);
        v.first_pixel[i] = R(c.first_pixel[i]);
        v.pdu[i] = R(c.pixel_delta_u[i]);
        v.pdv[i] = R(c.pixel_delta_v[i]);
        v.basis_u[i] = R(c.basis_u[i]);
        v.basis_v[i] = R(c.basis_v[i]);
    }
    v.aperture_radius = R(c.aperture_radius);
    v.inv_sqrt_spt = R(1.0 / double(p.sqrt_spt));  // camera.rs:52
    v.has_aperture = int32_t(c.has_aperture);
    v.width = c.image_width;
    v.height = c.image_height;
    v.sqrt_spt = p.sqrt_spt;
    v.thread_count = p.thread_count;
    v.max_depth = p.max_depth;
    return v;
}

template <typename R> ParamsView<R> make_params_view(const RtRenderParams& p, uint32_t owned) {
    ParamsView<R> v{};
    v.light_bias = R(p.light_bias);
    for (int i = 0; i < 3; i++) v.background[i] = p.has_background ? R(p.background[i]) : R(0);
    v.seed = p.seed;
    v.band_rows = p.band_rows;
    v.n_parts = p.n_parts;
    v.part = p.part;
    v.owned_rows = owned;
    v.spp = double(p.sqrt_spt) * double(p.sqrt_spt) * double(p.thread_count);  // camera.rs:50-51
    v.inv_spp = 1.0 / v.spp;
    return v;
}

// Both drivers render the replicas [t_first, t_first + n) of the frame `p` describes (T = p.thread_count) into d_out,
// which holds the running sum of [0, t_first) on entry when t_first > 0 (include/rt_mi355.h, RtAccum); a whole frame is
// t_first = 0, n = T.
template <typename R>
int render_typed(RtScene* s, DeviceScene<R>& ds, const RtCameraDesc& cam, const RtRenderParams& p, uint32_t owned,
                 uint32_t t_first, uint32_t n, double* d_out, hipStream_t stream) {
    CameraView<R> cv = make_camera_view<R>(cam, p);
    ParamsView<R> pv = make_params_view<R>(p, owned);
    const uint32_t tiles_x = (cam.image_width + 15u) / 16u, tiles_y = (owned + 15u) / 16u;
    const dim3 grid(tiles_x * tiles_y), block(256);
    const size_t lds = size_t(ds.view.stack_entries) * 256 * sizeof(int);
    if (lds > 160 * 1024) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the LDS traversal stack");
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, sizeof(DeviceCounters), stream));
    HIP_TRY(hipEventRecord(s->ev0, stream));
    // full-feature variant: texture interpreter (lerp / image / noise / channel / normal maps) and volumes
    const bool tex = s->compiled.needs_tex_interpreter || !s->compiled.volumes.empty();
#define RT_LAUNCH_MEGA(ST, TX) hipLaunchKernelGGL((k_megakernel<R, ST, TX>), grid, block, lds, stream, ds.view, cv, pv, d_out, s->d_counters.get(), t_first, n)
    if (p.collect_stats) { if (tex) RT_LAUNCH_MEGA(true, true); else RT_LAUNCH_MEGA(true, false); }
    else { if (tex) RT_LAUNCH_MEGA(false, true); else RT_LAUNCH_MEGA(false, false); }
#undef RT_LAUNCH_MEGA
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    DeviceCounters hc{};
    HIP_TRY(hipMemcpy(&hc, s->d_counters, sizeof hc, hipMemcpyDeviceToHost));
    RtRenderStats& st = s->stats;
    st = RtRenderStats{};
    st.kernel_ms = ms;
    st.traversal_kernel_ms = ms;
    st.n_launches = 1;
    st.pipeline_used = RT_PIPELINE_MEGAKERNEL;
    st.samples = uint64_t(cam.image_width) * owned * p.sqrt_spt * p.sqrt_spt * n;
    st.rays = hc.rays;
    st.mesh_rays = hc.mesh_rays;
    st.node_visits = hc.node_visits;
    st.tri_tests = hc.tri_tests;
    st.prim_tests = hc.prim_tests;
    st.bytes_node = sizeof(BvhNode<R>);
    st.bytes_tri = sizeof(TriRec<R>);
    st.bytes_attr = sizeof(TriAttr<R>);
    st.bytes_state = 0;
    return RT_OK;
}

// First-hit AOVs of the replicas [0, n) (rt_aov.hip): same tables, views and kernel variant as render_typed, but no
// counters, events or stats, so rt_get_stats still reports the last render.
template <typename R>
int aov_typed(RtScene* s, DeviceScene<R>& ds, const RtCameraDesc& cam, const RtRenderParams& p, uint32_t owned, uint32_t n,
              double* d_out, hipStream_t stream) {
    if (size_t(ds.view.stack_entries) * 256 * sizeof(int) > 160 * 1024) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the LDS traversal stack");
    const bool tex = s->compiled.needs_tex_interpreter || !s->compiled.volumes.empty();
    HIP_TRY(aov_launch<R>(ds.view, make_camera_view<R>(cam, p), make_params_view<R>(p, owned), tex, n, d_out, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// Wavefront pipeline driver
// ---------------------------------------------------------------------------------------------
constexpr size_t kSlabsMinTriangles = 131072;  // RT_WF_SLABS unset: the f64 kernels run the slab step if the scene's largest mesh has at least this many triangles

// ---- Kernel selection.  Taking a kernel's address instantiates it, so each selector names exactly the variants the
// library ships (tools/kernel_regs.py lists them) and a combination outside that set cannot be asked for.  Whoever needs a
// kernel twice (occupancy query and launch, render and ray query) keeps the pointer a selector returned. ----
template <typename R> using IntersectKernel = decltype(&k_wf_intersect<R, false, false>);
template <typename R> using PrimsKernel = decltype(&k_wf_prims<R, false, 0, false, false>);
template <typename R> using MeshKernel = decltype(&k_wf_mesh<R, false, 1, false>);
template <typename R, typename G> using ShadeKernel = decltype(&k_wf_shade<R, false, 0, false, G, false>);

template <typename R>
IntersectKernel<R> pick_intersect(bool stats, bool vol) {
    if (stats) return vol ? &k_wf_intersect<R, true, true> : &k_wf_intersect<R, true, false>;
    return vol ? &k_wf_intersect<R, false, true> : &k_wf_intersect<R, false, false>;
}

// lds: 0 = tables from global memory, 1 = all staged, 2 = a prefix.  Volumes: no staged tables, no group BVHs.
template <typename R, bool ST>
PrimsKernel<R> pick_prims_st(bool vol, bool groups, int lds) {
    if (vol) return &k_wf_prims<R, ST, 0, true, false>;
    if (groups) return lds == 2 ? &k_wf_prims<R, ST, 2, false, true> : (lds == 1 ? &k_wf_prims<R, ST, 1, false, true> : &k_wf_prims<R, ST, 0, false, true>);
    return lds == 2 ? &k_wf_prims<R, ST, 2, false, false> : (lds == 1 ? &k_wf_prims<R, ST, 1, false, false> : &k_wf_prims<R, ST, 0, false, false>);
}
template <typename R>
PrimsKernel<R> pick_prims(bool stats, bool vol, bool groups, int lds) {
    return stats ? pick_prims_st<R, true>(vol, groups, lds) : pick_prims_st<R, false>(vol, groups, lds);
}

template <typename R, bool ST>
MeshKernel<R> pick_mesh_st(int node_kind, bool multi, bool slabs) {
    if constexpr (sizeof(R) == 8) {  // the form with the slab step: f64, quantised nodes
        if (node_kind == 1 && slabs) return multi ? &k_wf_mesh<R, ST, 1, true, true> : &k_wf_mesh<R, ST, 1, false, true>;
    }
    if (node_kind == 1) return multi ? &k_wf_mesh<R, ST, 1, true> : &k_wf_mesh<R, ST, 1, false>;
    return multi ? &k_wf_mesh<R, ST, 0, true> : &k_wf_mesh<R, ST, 0, false>;
}
template <typename R>
MeshKernel<R> pick_mesh(bool stats, int node_kind, bool multi, bool slabs) {
    return stats ? pick_mesh_st<R, true>(node_kind, multi, slabs) : pick_mesh_st<R, false>(node_kind, multi, slabs);
}

// k_wf_shade of a group type G.  Every G has the lean variants (interpreter variant: tables from global memory - rare scenes,
// fewer instantiations).  The fused kernel (+ k_wf_prims' search as phase 4) exists for the groups whose restarts leave it the
// registers: WfGroup, WfGroupRays, WfGroupPoints, WfGroupProbes.  The counting variants exist for WfGroup alone; a caller whose G has none
// refuses collect_stats before it comes here.
template <typename G> constexpr bool kShadeFused = !G::kSparse && !G::kLightGroups;
template <typename R, typename G, bool ST>
ShadeKernel<R, G> pick_shade_st(int lds, bool tex) {
    if (tex) return &k_wf_shade<R, ST, 0, true, G>;
    return lds == 1 ? &k_wf_shade<R, ST, 1, false, G> : (lds == 2 ? &k_wf_shade<R, ST, 2, false, G> : &k_wf_shade<R, ST, 0, false, G>);
}
template <typename R, typename G>
ShadeKernel<R, G> pick_shade(bool stats, int lds, bool tex, bool fuse) {
    if constexpr (kShadeFused<G>) if (fuse) return &k_wf_shade<R, false, 1, false, G, true>;
    if (!stats) return pick_shade_st<R, G, false>(lds, tex);
    return pick_shade_st<R, G, std::is_same_v<G, WfGroup<R>>>(lds, tex);  // no counting variants for the other groups: their modes refuse collect_stats
}

// ---- Search setup: which of k_wf_prims / k_wf_mesh / k_wf_intersect serve a scene, and with which grid, LDS and
// arguments.  Built by make_search_setup for renders and ray queries alike, which is what makes a query's answers the
// render's hits; every switch below is read there and nowhere else. ----
template <typename R>
struct SearchSetup {
    WavefrontPlan plan;
    bool stats, vol;
    bool use_split, prims_only, split;  // split: k_wf_prims + k_wf_mesh; prims_only: no mesh ops; neither: k_wf_intersect
    bool multi_mesh;
    int node_kind;
    uint32_t cones_on;
    uint32_t slabs_on;  // RT_WF_SLABS: 0 off, 1 every child (default), 2 leaf children only
    int mesh_levels, lds_levels;        // k_wf_mesh's stack: levels in all / in LDS (the rest in the workspace's spill buffer)
    uint32_t refill_min, inner_min;
    HandoutPolicy handout;              // how the persistent kernels' waves share their queue (rt_handout.h)
    bool lds_tables;                    // RT_LDS_TABLES / RT_LDS_BUDGET, for staged_prefix of the shade kernel's layout too
    uint32_t lds_budget;
    bool groups;
    uint32_t group_levels;
    size_t lds_groups;
    uint32_t staged_prims;
    int lds_prims;                      // kernel variant: none / all / prefix
    size_t lds_isect, lds_mesh, lds_prims_launch;  // dynamic LDS of each launch
    uint32_t isect_blocks;              // persistent grid of k_wf_mesh / k_wf_intersect
    int blocks_per_cu;                  // ... what the occupancy query gave for it
    size_t spill_bytes;                 // what the workspace's mesh_spill must hold (0: no k_wf_mesh)
    IntersectKernel<R> k_intersect;
    PrimsKernel<R> k_prims;
    MeshKernel<R> k_mesh;
};

// small tables staged in LDS by the prims / shade kernels: the longest prefix of whole tables (in the kernel's own table order)
// that fits the budget; 32 KB keeps four workgroups per CU resident next to the queue lists
static uint32_t staged_prefix(const SmallLayout& L, bool lds_tables, uint32_t lds_budget) {
    if (!lds_tables) return 0u;
    if (L.total_bytes <= lds_budget) return L.total_bytes;
    uint32_t best = 0;  // tables are packed back to back in staging order: a table fits iff its end does
    for (int k = 0; k < ST_COUNT; k++)
        if (L.end[k] <= lds_budget && L.end[k] > best) best = L.end[k];
    return (best + 15u) & ~15u;
}

// vol: volume ops (combined intersect kernel or k_wf_prims, VOL variant); ray queries have none.
template <typename R>
int make_search_setup(RtScene* s, DeviceScene<R>& ds, bool stats, bool vol, SearchSetup<R>* out) {
    SearchSetup<R>& su = *out;
    su.stats = stats;
    su.vol = vol;
    su.lds_isect = size_t(ds.view.stack_entries) * 256 * sizeof(int);
    if (su.lds_isect > 160 * 1024) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the LDS traversal stack");
    // which kernels serve this scene (rt_compile.cpp plan_wavefront); RT_WF_SPLIT=0 (tests): the combined kernel for every scene
    su.plan = plan_wavefront(s->compiled);
    const int n_mesh_ops = int(s->compiled.mesh_ops.size());
    su.use_split = env_u32("RT_WF_SPLIT", 1) != 0 && su.plan.split;
    su.prims_only = su.use_split && n_mesh_ops == 0;
    su.split = su.use_split && n_mesh_ops > 0;
    su.multi_mesh = su.plan.multi_mesh || env_u32("RT_WF_MESH_MULTI", 0) != 0;  // the general form of k_wf_mesh (env: A/B on single-mesh scenes, tests)
    // k_wf_mesh keeps (child, entry distance) pairs: a shallow LDS part (occupancy) + a global spill part
    // BVH node format of k_wf_mesh: 1 = 4-wide quantised (BvhNode4q, 64 B, default), 0 = 4-wide f32 (BvhNode4f, 128 B; A/B control).
    // An 8-wide quantised node (a third fewer visits) was slower: profiles/r02/ab/node_width_and_size.txt.
    su.node_kind = env_u32("RT_WF_NODES", 1) != 0 ? 1 : 0;
    // Back-face cone test of the quantised node step: 0 = off (A/B control: the same code object, never-culling direction word).
    su.cones_on = env_u32("RT_WF_CONES", 1) != 0 ? 1u : 0u;
    // Normal-slab test behind the box test (the SLABS forms of k_wf_mesh): RT_WF_SLABS = 0 off, 1 every child, 2 leaf children only.
    // f64 and quantised nodes only: in f32 the step is not result-preserving (the f32 triangle test accepts a few rays per 10^9
    // that pass a triangle farther off than the slab's margin: 2 pixels of the headline frame changed), so there is no f32 form and
    // the variable is ignored there.  Unset: every child if the scene's LARGEST mesh has at least kSlabsMinTriangles triangles, off
    // otherwise.  Measured (profiles/mesh_slabs/README.md), k_wf_mesh against the parent's: -11.9 % on the 871 200-triangle headline
    // mesh, -16 % on the 3.5 M-triangle one, -1.6 % and -3 % on Suzanne (15.7 k, c3 and c1), +3.7 % on the 1 k-triangle meshes of
    // two_meshes (shallow trees: few visits to save, the step's instructions on every one).  On Suzanne the frame does not move
    // (inside its spread), so the threshold stays above it, where the frame gains: between 15.7 k and 871 k nothing is measured.
    // The setting is one per launch: a scene with one large and many small meshes runs the
    // step on all of them.
    size_t largest_mesh = 0;
    for (const MeshInst& mi : s->compiled.meshes) largest_mesh = std::max(largest_mesh, size_t(mi.n_tris));
    const uint32_t slabs_dflt = largest_mesh >= kSlabsMinTriangles ? 1u : 0u;
    su.slabs_on = (sizeof(R) == 8 && su.node_kind == 1) ? std::min(env_u32("RT_WF_SLABS", slabs_dflt), 2u) : 0u;
    su.mesh_levels = int(s->compiled.max_bvh4_stack) + 1;
    su.lds_levels = std::min<int>(su.mesh_levels, int(env_u32("RT_WF_LDS_LEVELS", 12)));
    su.lds_mesh = size_t(su.lds_levels) * 256 * sizeof(uint2) + 4 * kMeshWaveLds<R>;
    su.refill_min = env_u32("RT_WF_REFILL", 32);  // measured optimum (64 = no refill: -20 %)
    su.inner_min = env_u32("RT_WF_INNER_MIN", 24);  // 16 / 24 / 32: 982 / 973 / 1013 ms on the headline, 766 / 758 / 784 in f32 (profiles/mesh_handout/sweep_inner_min.txt)
    // RT_WF_HANDOUT: 0 = 256 entries per atomic from the first on (A/B control, the same code object), 1 = static first range +
    // shrinking ranges, 2 = 1 + queue entries staged in LDS by k_wf_mesh.  RT_WF_HANDOUT_256 / _128: the policy's thresholds (sweeps).
    su.handout.mode = std::min<uint32_t>(env_u32("RT_WF_HANDOUT", 2), 2u);
    su.handout.left256 = env_u32("RT_WF_HANDOUT_256", kHandoutLeft256);
    su.handout.left128 = std::min<uint32_t>(env_u32("RT_WF_HANDOUT_128", kHandoutLeft128), su.handout.left256);
    su.lds_tables = env_u32("RT_LDS_TABLES", 1) != 0;
    su.lds_budget = env_u32("RT_LDS_BUDGET", 32u * 1024u);
    // re-built primitive groups as 4-wide BVHs inside k_wf_prims (OP_GROUP): nodes + a per-lane stack in LDS; scenes whose
    // groups need more than that LDS (> 24 KB of nodes, > 16 stack levels) keep the op form.  RT_WF_GROUPS=0: A/B, tests.
    su.group_levels = uint32_t(ds.view.group_stack_levels);
    const size_t group_node_bytes = size_t(ds.view.n_group_nodes) * sizeof(BvhNode4q);
    su.groups = (su.split || su.prims_only) && su.plan.groups && env_u32("RT_WF_GROUPS", 1) != 0;
    su.lds_groups = su.groups ? size_t(su.group_levels) * 256 * 8 + group_node_bytes : 0;
    su.staged_prims = staged_prefix(ds.view.lay, su.lds_tables, su.lds_budget);
    if (su.groups && su.lds_groups + su.staged_prims > 44u * 1024u) su.staged_prims = 0;  // three workgroups per CU with the group data: tables from global memory
    su.lds_prims = su.staged_prims == 0 ? 0 : (su.staged_prims == ds.view.lay.total_bytes ? 1 : 2);
    su.lds_prims_launch = (vol ? size_t(0) : size_t(su.staged_prims) + su.lds_groups) + (WF_CHUNK + 4) * 4;
    su.k_intersect = pick_intersect<R>(stats, vol);
    su.k_prims = pick_prims<R>(stats, vol, su.groups, su.lds_prims);
    su.k_mesh = pick_mesh<R>(stats, su.node_kind, su.multi_mesh, su.slabs_on != 0u);
    // persistent grids: as many workgroups as stay resident.  The combined kernel's grid is the lean variant's at either
    // setting of `stats`; k_wf_mesh's is the launched variant's own.
    int n_cu = 0, blocks_per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device));
    if (su.split) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, su.k_mesh, 256, su.lds_mesh));
    else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, pick_intersect<R>(false, vol), 256, su.lds_isect));
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    if (su.split) blocks_per_cu = std::min<int>(blocks_per_cu, int(env_u32("RT_WF_MESH_BLOCKS", 64)));  // experiments: occupancy scaling
    su.isect_blocks = uint32_t(n_cu) * uint32_t(blocks_per_cu);
    su.blocks_per_cu = blocks_per_cu;
    if (const uint32_t grid = env_u32("RT_WF_MESH_GRID", 0)) su.isect_blocks = std::min<uint32_t>(grid, 16384u);  // tests, A/B: the persistent grid outright
    su.spill_bytes = su.split ? size_t(std::max(su.mesh_levels - su.lds_levels, 1)) * su.isect_blocks * 256 * sizeof(uint2) : size_t(0);
    return RT_OK;
}

// The search launches of one pass over a queue, on a workspace's queues and counters (RtScene::Wavefront or ::Query).
struct SearchQueues {
    const uint32_t* queue;
    uint32_t* mesh_queue;
    void* mesh_spill;
    WfCounters* ctr;
    DeviceCounters* counters;
    hipStream_t stream;
};
// k_wf_prims over the first n_queued entries (an upper bound) of sq.queue; fills sq.mesh_queue
template <typename R>
void launch_prims(const SearchSetup<R>& su, const DeviceScene<R>& ds, const WfPool<R>& pool, const SearchQueues& sq, uint32_t n_queued) {
    hipLaunchKernelGGL(su.k_prims, dim3((n_queued + WF_CHUNK - 1) / WF_CHUNK), dim3(256), su.lds_prims_launch, sq.stream, ds.view, pool, sq.queue,
                       sq.mesh_queue, sq.ctr, sq.counters, su.staged_prims, su.group_levels);
}
template <typename R>
void launch_mesh(const SearchSetup<R>& su, const DeviceScene<R>& ds, const WfPool<R>& pool, const SearchQueues& sq) {
    hipLaunchKernelGGL(su.k_mesh, dim3(su.isect_blocks), dim3(256), su.lds_mesh, sq.stream, ds.view, pool, sq.mesh_queue, sq.ctr, sq.counters,
                       su.refill_min, su.inner_min, static_cast<uint2*>(sq.mesh_spill), su.lds_levels, &sq.ctr->n_mesh, &sq.ctr->cursor, su.cones_on, su.slabs_on, su.handout.mode, su.handout.left256, su.handout.left128);
}
template <typename R>
void launch_intersect(const SearchSetup<R>& su, const DeviceScene<R>& ds, const WfPool<R>& pool, const SearchQueues& sq) {
    hipLaunchKernelGGL(su.k_intersect, dim3(su.isect_blocks), dim3(256), su.lds_isect, sq.stream, ds.view, pool, sq.queue, sq.ctr, sq.counters,
                       su.refill_min, su.handout.mode, su.handout.left256, su.handout.left128);
}

// Builds `pl` for `capacity` slots: rays and hit records, `full`: + the rest of the path state and the descriptor's device
// copy; n_queues queues and (with any queue) the mesh queue.  Every allocation maps out-of-memory to RT_E_NOMEM with the
// message `nomem`; a failure leaves an empty pool behind and never a half-built one.  RT_WF_FAKE_OOM_ABOVE (tests): above
// that many slots the LAST allocation fails like hipErrorOutOfMemory, with everything before it in place.
template <typename R>
int build_pool(PathPool<R>& pl, uint32_t capacity, bool full, int n_queues, const char* nomem) {
    pl = PathPool<R>{};
    WfPool<R>& v = pl.view;
    v.capacity = capacity;
    std::vector<std::pair<void**, size_t>> want;  // where the pointer goes, bytes
    auto per_slot = [&](auto** at, size_t each) { want.emplace_back(reinterpret_cast<void**>(at), size_t(capacity) * each); };
    for (R** r : {&v.ox, &v.oy, &v.oz, &v.dx, &v.dy, &v.dz, &v.ht, &v.hu, &v.hv}) per_slot(r, sizeof(R));
    per_slot(&v.hpc, 4);
    per_slot(&v.htri, 4);
    if (full) {
        for (R** r : {&v.tr, &v.tg, &v.tb}) per_slot(r, sizeof(R));
        per_slot(&v.rng, 8);
        per_slot(&v.sample, 8);
        per_slot(&v.depth, 4);
    }
    for (int q = 0; q < n_queues; q++) per_slot(&pl.queue[q], 4);
    if (n_queues) per_slot(&pl.mesh_queue, 4);
    if (full) want.emplace_back(reinterpret_cast<void**>(&pl.dev), sizeof(WfPool<R>));
    const uint32_t limit = env_u32("RT_WF_FAKE_OOM_ABOVE", 0);
    int st = RT_OK;
    for (size_t i = 0; i < want.size() && st == RT_OK; i++) {
        pl.owned.emplace_back();
        if (limit && capacity > limit && i + 1 == want.size()) st = set_err(RT_E_NOMEM, std::string(nomem) + " (RT_WF_FAKE_OOM_ABOVE)");
        else st = pl.owned.back().reserve(want[i].second, nomem);
        *want[i].first = pl.owned.back().get();
    }
    if (st == RT_OK && full)
        if (const hipError_t e = hipMemcpy(pl.dev, &v, sizeof v, hipMemcpyHostToDevice); e != hipSuccess) st = set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    if (st != RT_OK) pl = PathPool<R>{};
    return st;
}
template int build_pool<float>(PathPool<float>&, uint32_t, bool, int, const char*);  // rt_query.hip builds the query pool
template int build_pool<double>(PathPool<double>&, uint32_t, bool, int, const char*);

// The render's pools of exactly `capacity` slots in R, its counters and its timing events.
template <typename R>
int wf_ensure(RtScene* s, uint32_t capacity) {
    RtScene::Wavefront& w = s->wf;
    const auto* have = std::get_if<PoolPair<R>>(&w.pools);
    if (have && (*have)[0].view.capacity == capacity) return RT_OK;
    w.pools = std::monostate{};  // released before the new ones are built; a failure below leaves the pool absent
    const char* nomem = "path pool does not fit in device memory";
    if (int st = w.d_ctr.reserve(sizeof(WfCounters), nomem)) return st;
    if (int st = w.h_ctr.reserve(sizeof(WfCounters), nomem)) return st;
    w.events.resize(136);  // 4 per iteration, up to 32 iterations between host checks, + 2 for the stand-alone prims launch
    for (Event& e : w.events)
        if (int st = e.ensure()) return st;
    PoolPair<R> pp;
    if (int st = build_pool(pp[0], capacity, true, 2, nomem)) return st;
    // a compaction happens below RT_WF_COMPACT_PCT <= 75 % of the addressed slots
    if (int st = build_pool(pp[1], std::max<uint32_t>(64u, uint32_t((uint64_t(capacity) * 3 + 3) / 4)), true, 0, nomem)) return st;
    w.pools = std::move(pp);
    return RT_OK;
}

// ---- Render modes.  A call of render_wavefront has exactly one: a plain frame, a dense or a sparse adaptive pass, a light-group
// render, a ray table, a point table or a probe table.  The mode type says what the driver must not know: its replica-group type Group<R>
// (k_wf_generate and k_wf_shade are instantiated per group type) and how one is completed from the common base the driver
// fills (`complete`); how many pixels a group covers (`npix`); the refusal collect_stats meets (`kNoCounting`; null: the mode
// has counting kernels); whether every sample has an origin of its own (`kOwnOrigins`); what a sample takes in device memory
// and what else the call needs there (`kSampleBytes`, `reserve`); whether several groups keep running sums in
// w.acc (`kRunningSums`); and how a finished replica group is resolved (`resolve`).  PassBase answers as a plain frame does. ----
// A finished replica group as `resolve` sees it: nrep replicas of npix pixels in w.sample_L.  first / last: the call's first /
// last group; resumed: the call continues a running sum in d_out.
struct WfResolve {
    RtScene::Wavefront& w;
    uint64_t npix;
    uint32_t strata, nrep, T, tid0;  // tid0: the group's first replica
    double spp, *d_out;
    int first, resumed, last;
    hipStream_t stream;
};
struct PassBase {
    template <typename R> using Group = WfGroup<R>;
    static constexpr const char* kNoCounting = nullptr;
    static constexpr bool kOwnOrigins = false, kRunningSums = true;
    static constexpr uint32_t kSampleBytes = 24;  // radiance; what a mode adds to it lives in w.sample_G
    uint64_t npix(uint64_t frame) const { return frame; }
    int reserve(RtScene::Wavefront&, uint64_t, uint64_t, uint32_t, uint32_t, hipStream_t) const { return RT_OK; }  // (w, per_replica, npix, group, n, stream)
    template <typename G> void complete(G&, RtScene::Wavefront&) const {}
    int resolve(const WfResolve& a) const {
        hipLaunchKernelGGL(k_wf_resolve, dim3(uint32_t((a.npix + 255) / 256)), dim3(256), 0, a.stream, a.w.sample_L.get(), a.w.acc.get(), a.npix, a.strata,
                           a.nrep, a.spp, a.first, a.resumed, a.d_out, a.last);
        return RT_OK;
    }
};
struct FramePass : PassBase {};

// The two modes of an AdaptivePass (rt_render.h), dense and sparse.
template <bool SPARSE>
struct AdaptiveMode : AdaptivePass, PassBase {
    template <typename R> using Group = std::conditional_t<SPARSE, WfGroupSparse<R>, WfGroup<R>>;
    static constexpr const char* kNoCounting = "adaptive passes have no counting kernels (collect_stats)";
    static constexpr bool kRunningSums = false;  // every group resolves into the accumulator's sums
    uint64_t npix(uint64_t frame) const { return SPARSE ? uint64_t(n_active) : frame; }
    template <typename G> void complete(G& g, RtScene::Wavefront&) const { if constexpr (SPARSE) g.active = active; }
    int resolve(const WfResolve& a) const {
        hipLaunchKernelGGL(k_wf_resolve_moments<SPARSE>, dim3(uint32_t((a.npix + 255) / 256)), dim3(256), 0, a.stream, a.w.sample_L.get(), a.npix, a.strata,
                           a.nrep, a.spp, double(a.T), active, a.d_out, s1, s2, cnt);
        return RT_OK;
    }
};

// A light-group render (rt_render_light_groups): k_wf_shade records the group of every terminal and
// k_wf_resolve_groups sums per group.  `table` (host): n_materials + 2 bytes as WfGroupLG describes them.  d_out (the
// ordinary frame, through the unchanged k_wf_resolve) may be NULL.
// launch() between the workspace's two resolve events, then a synchronise: its milliseconds are added to *ms_sum.
template <typename F>
int timed_resolve(const WfResolve& a, double* ms_sum, F&& launch) {
    HIP_TRY(hipEventRecord(a.w.ev_res[0], a.stream));
    if (int st = launch()) return st;
    HIP_TRY(hipEventRecord(a.w.ev_res[1], a.stream));
    HIP_TRY(hipStreamSynchronize(a.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a.w.ev_res[0], a.w.ev_res[1]));
    *ms_sum += ms;
    return RT_OK;
}

struct LightGroupPass : PassBase {
    uint32_t n_groups = 0, n_materials = 0;
    const uint8_t* table = nullptr;
    double* d_groups_out = nullptr;
    mutable double resolve_ms = 0;  // both resolve kernels, summed over the call's groups (RT_LG_LOG)
    template <typename R> using Group = WfGroupLG<R>;
    static constexpr const char* kNoCounting = "light groups have no adaptive or counting kernels (collect_stats)";
    static constexpr uint32_t kSampleBytes = 25;  // + the group byte
    int reserve(RtScene::Wavefront& w, uint64_t per_replica, uint64_t npix, uint32_t group, uint32_t n, hipStream_t stream) const {
        if (int st = w.sample_G.reserve(size_t(per_replica) * group)) return st;
        if (int st = w.acc_g.reserve(group < n ? size_t(npix) * 24 * n_groups : size_t(0))) return st;
        const size_t need_t = size_t(n_materials) + 2;
        if (int st = w.lg_table.reserve(need_t)) return st;
        HIP_TRY(hipMemcpyAsync(w.lg_table, table, need_t, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // the host table may be the caller's stack
        for (Event& e : w.ev_res)
            if (int st = e.ensure()) return st;
        return RT_OK;
    }
    template <typename G> void complete(G& g, RtScene::Wavefront& w) const { g.sample_G = w.sample_G; g.table = w.lg_table; g.n_materials = n_materials; }
    int resolve(const WfResolve& a) const {
        if (int st = timed_resolve(a, &resolve_ms, [&]() -> int {
                if (a.d_out) PassBase::resolve(a);
                const uint64_t blocks = ((a.npix + 63) / 64) * ((n_groups + 3u) / 4u);
                if (blocks > 0x7FFFFFFFull) return set_err(RT_E_UNSUPPORTED, "frame too large for the light-group resolve");
                hipLaunchKernelGGL(k_wf_resolve_groups, dim3(uint32_t(blocks)), dim3(256), 0, a.stream, a.w.sample_L.get(), a.w.sample_G.get(), a.w.acc_g.get(),
                                   a.npix, n_groups, a.strata, a.nrep, a.spp, a.first, d_groups_out, a.last);
                return RT_OK;
            }))
            return st;
        if (a.last && env_u32("RT_LG_LOG", 0))  // tools/gpu_light_groups_cost.py
            std::fprintf(stderr, "[light groups] G %u: resolve kernels %.3f ms, %zu B of group bytes, %zu B of group sums\n", n_groups, resolve_ms,
                         a.w.sample_G.bytes(), a.w.acc_g.bytes());
        return RT_OK;
    }
};

// What the table modes share: a call renders one chunk of the caller's table as a "frame" of n x 1
// pixels, pixel i = entry first + i, and every sample starts where its entry says.  table_render_check refuses collect_stats
// before a pass exists.
struct TablePass : PassBase {
    uint64_t first = 0;
    static constexpr const char* kNoCounting = "table modes have no adaptive, light-group or counting kernels (collect_stats)";
    static constexpr bool kOwnOrigins = true;
};

// A render along a ray table (rt_render_rays): origins / dirs are device pointers to the chunk's first ray.
struct RayTablePass : TablePass {
    const double* origins = nullptr;
    const double* dirs = nullptr;
    template <typename R> using Group = WfGroupRays<R>;
    template <typename G> void complete(G& g, RtScene::Wavefront&) const { g.origins = origins; g.dirs = dirs; g.first = first; }
};

// An irradiance bake (rt_bake_irradiance): pos / nrm are device pointers to the chunk's first position and
// normal, `stride` bytes apart from point to point (24: plain arrays; sizeof(RtRayHit): hit records).
struct PointTablePass : TablePass {
    const unsigned char* pos = nullptr;
    const unsigned char* nrm = nullptr;
    uint32_t stride = 24;
    template <typename R> using Group = WfGroupPoints<R>;
    template <typename G> void complete(G& g, RtScene::Wavefront&) const { g.pos = pos; g.nrm = nrm; g.stride = stride; g.first = first; }
};

// An SH probe bake (rt_bake_probes): pos is a device pointer to the chunk's first position.  The resolve
// weights every sample by the SH basis of its first direction, re-derived from the sample's key (k_wf_resolve_sh): d_out is
// n x 9 x 4 doubles, and several replica groups carry 27 doubles per probe in w.acc instead of a pixel's 3.
struct ProbeTablePass : TablePass {
    const double* pos = nullptr;
    uint64_t seed = 0;
    uint32_t S = 1;
    bool f32 = false;
    template <typename R> using Group = WfGroupProbes<R>;
    static constexpr bool kRunningSums = false;  // the sums between groups are this mode's own size
    int reserve(RtScene::Wavefront& w, uint64_t, uint64_t npix, uint32_t group, uint32_t n, hipStream_t) const {
        return w.acc.reserve(group < n ? size_t(npix) * 27 * sizeof(double) : size_t(0));
    }
    template <typename G> void complete(G& g, RtScene::Wavefront&) const { g.pos = pos; g.first = first; }
    template <typename R> void launch_resolve(const WfResolve& a, uint32_t tid0) const {
        hipLaunchKernelGGL((k_wf_resolve_sh<R>), dim3(uint32_t(((a.npix + 63) / 64) * 3u)), dim3(256), 0, a.stream, a.w.sample_L.get(), a.w.acc.get(), a.npix, first,
                           seed, tid0, S, R(1.0 / double(S)), a.nrep, a.spp, a.first, a.d_out, a.last);
    }
    mutable double resolve_ms = 0;  // k_wf_resolve_sh, summed over the chunk's groups (RT_PROBES_LOG)
    int resolve(const WfResolve& a) const {
        auto launch = [&]() -> int {
            if (f32) launch_resolve<float>(a, a.tid0);
            else launch_resolve<double>(a, a.tid0);
            return RT_OK;
        };
        if (!env_u32("RT_PROBES_LOG", 0)) return launch();
        // tools/gpu_bake_probes_cost.py: times the resolve with events, at the price of a synchronise per group
        for (Event& e : a.w.ev_res)
            if (int st = e.ensure()) return st;
        if (int st = timed_resolve(a, &resolve_ms, launch)) return st;
        if (a.last) std::fprintf(stderr, "[probes] %llu probes from %llu on, %u paths each: k_wf_resolve_sh %.3f ms\n", (unsigned long long)a.npix, (unsigned long long)first, a.strata * a.T, resolve_ms);
        return RT_OK;
    }
};

// Pool size of a render.  Every launch of the persistent mesh kernel ends with a drain of ~0.4 ms (the longest remaining traversals:
// dependent fetches) and the streaming kernels run better in few large launches, so fewer, larger launches win; against that
// stands the tail: the pool is what drains at the end of a replica group, over ~20 ever smaller iterations.  Round 2 (tail at
// 2.5 x its work's worth): best size 64 M slots at 1.44 G samples, growing with the square root of the work.  Round 3's tail
// compaction (k_wf_compact) halved the tail's price and moved the optimum up - Msamples/s, same box (profiles/r03/tail_compaction.txt):
//   C4 1.44 G samples:  64 M 1256-1287, 96 M 1289-1293, 128 M 1312-1332, 160 M 1319-1338, 192 M 1326-1337, 256 M 1300-1311
//   C3 0.96 G: 52 M 4841, 80 M 4907, 96 M 4977, 112 M 4890      C1 0.25 G: 26 M 1962, 48 M 2028, 64 M 2061-2079, 96 M 2120, 128 M 2129
//   C2 0.16 G (no mesh): 16 M 1681, 22 M 1692, 32 M 1668, 44 M 1670      one of 8 ranks' share of C4: 23 M 157 ms, 46 M / 92 M 151, 128 M 153
// -> 128 M slots at 1.44 G samples, with the square root of the work below it (within 1-3 % of each workload's best).
// Sized from the whole frame (T replicas), not from this call's n: progressive passes of any size keep the same pool.
static uint32_t wf_pool_capacity(uint32_t strata, uint64_t npix_frame, uint32_t T) {
    const double total_samples = double(strata) * double(npix_frame) * double(T);  // the frame's, also for a sparse pass: one pool for all passes
    double c = 134217728.0 * std::sqrt(total_samples / 1.44e9);
    c = std::fmin(std::fmax(c, 1048576.0), 134217728.0);
    uint32_t capacity = env_u32("RT_WF_POOL", uint32_t(c) & ~0xFFFFFu);
    if (capacity > (1u << 28)) capacity = 1u << 28;  // the kernels address pool arrays through 32-bit byte offsets (rt_wavefront.h, at())
    if (uint64_t(capacity) > uint64_t(strata) * npix_frame * T) capacity = uint32_t(uint64_t(strata) * npix_frame * T);
    return std::max<uint32_t>(capacity, 64u);
}

// The per-sample buffers' plan of a call that renders n replicas of per_replica samples each: *group_out = replicas per group,
// as many as the memory budget allows at sample_bytes per sample (24 of radiance in sample_L; a mode's own bytes in sample_G),
// sample_L for them, and the running sums between several groups if the mode keeps any (grow only).
static int wf_plan_samples(RtScene::Wavefront& w, uint64_t per_replica, uint64_t npix, uint32_t n, uint32_t sample_bytes, bool running_sums,
                           uint32_t* group_out) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    size_t budget = size_t(env_u32("RT_WF_SAMPLE_GB", 64)) << 30;
    size_t avail = free_b + w.sample_L.bytes() + (sample_bytes > 24 ? w.sample_G.bytes() : size_t(0));
    if (budget > avail / 2) budget = avail / 2;
    uint64_t bytes_per_replica = per_replica * sample_bytes;
    uint32_t group = uint32_t(std::min<uint64_t>(n, std::max<uint64_t>(1, budget / bytes_per_replica)));
    group = (n + (n + group - 1) / group - 1) / ((n + group - 1) / group);  // same number of groups, equal sizes (9 + 1 -> 5 + 5)
    if (bytes_per_replica > avail) return set_err(RT_E_NOMEM, "per-sample radiance buffer of one replica does not fit in device memory");
    if (int st = w.sample_L.reserve(size_t(per_replica) * 24 * group)) return st;
    if (group < n && running_sums)  // several groups: running sums between them
        if (int st = w.acc.reserve(size_t(npix) * 24)) return st;
    *group_out = group;
    return RT_OK;
}

// RT_WF_TRACE=n (debug): the queue and the first n slots of the pool after an iteration, on stderr.
template <typename R>
int wf_trace_dump(const WfPool<R>& pool, uint32_t first, const uint32_t* queue, uint32_t n_in, uint32_t iteration) {
    const uint32_t n = std::min<uint32_t>(std::min(first, pool.capacity), env_u32("RT_WF_TRACE", 0));
    std::vector<R> a[12];
    R* src[12] = {pool.ox, pool.oy, pool.oz, pool.dx, pool.dy, pool.dz, pool.tr, pool.tg, pool.tb, pool.ht, pool.hu, pool.hv};
    for (int k = 0; k < 12; k++) { a[k].resize(n); HIP_TRY(hipMemcpy(a[k].data(), src[k], n * sizeof(R), hipMemcpyDeviceToHost)); }
    std::vector<uint64_t> rngs(n), smp(n);
    std::vector<uint32_t> dep(n), qn(first);
    std::vector<int32_t> hpc(n);
    HIP_TRY(hipMemcpy(rngs.data(), pool.rng, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(smp.data(), pool.sample, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dep.data(), pool.depth, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hpc.data(), pool.hpc, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(qn.data(), queue, size_t(n_in) * 4, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[wf trace] iteration %u: %u paths queued:", iteration, n_in);
    for (uint32_t k = 0; k < n_in && k < 64; k++) std::fprintf(stderr, " %u", qn[k]);
    std::fprintf(stderr, "\n");
    for (uint32_t k = 0; k < n; k++)
        std::fprintf(stderr, "  slot %u sample %llu depth %u o %.17g %.17g %.17g d %.17g %.17g %.17g thr %.6g %.6g %.6g hit t %.17g pc %d rng %016llx\n", k,
                     (unsigned long long)smp[k], dep[k], double(a[0][k]), double(a[1][k]), double(a[2][k]), double(a[3][k]), double(a[4][k]),
                     double(a[5][k]), double(a[6][k]), double(a[7][k]), double(a[8][k]), double(a[9][k]), hpc[k], (unsigned long long)rngs[k]);
    return RT_OK;
}

// What the loop of render_wavefront counts and times.  phase_ms: HIP-event sums per kernel, 4 events per iteration (before
// prims / intersect, after it, after the mesh kernel, after shade); slot 0 = prims, 1 = traversal (mesh or combined
// intersect), 2 = shade.
struct WfTally {
    double phase_ms[3];
    uint32_t search_launches;    // stand-alone k_wf_prims / k_wf_intersect launches
    uint32_t iterations, n_groups, n_compactions;
};

// RtRenderStats of a wavefront render that has ended (ev0 .. ev1 of the scene span it), and its debug lines.
template <typename R>
int wf_fill_stats(RtScene* s, const SearchSetup<R>& su, const WfTally& ty, bool fusable, uint64_t samples) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    DeviceCounters hc{};
    HIP_TRY(hipMemcpy(&hc, s->d_counters, sizeof hc, hipMemcpyDeviceToHost));
    RtRenderStats& st = s->stats;
    st = RtRenderStats{};
    st.kernel_ms = ms;
    st.traversal_kernel_ms = su.prims_only ? 0.0 : ty.phase_ms[1];
    st.prims_kernel_ms = (su.split || su.prims_only) ? ty.phase_ms[0] : 0.0;
    st.shade_kernel_ms = ty.phase_ms[2];
    st.n_launches = ty.search_launches;
    st.n_iterations = ty.iterations;
    st.n_replica_groups = ty.n_groups;
    st.n_tail_compactions = ty.n_compactions;
    if (su.stats && su.split && env_u32("RT_WF_DEBUG", 0)) {
        std::fprintf(stderr, "[k_wf_mesh] grid %u workgroups, %d per CU, %zu B of LDS each; hand-out mode %u, 256 / 128 entries above %u / %u left per wave\n",
                     su.isect_blocks, su.blocks_per_cu, su.lds_mesh, su.handout.mode, su.handout.left256, su.handout.left128);
        auto pct = [](unsigned long long lanes, unsigned long long waves) { return waves ? 100.0 * double(lanes) / (64.0 * double(waves)) : 0.0; };
        std::fprintf(stderr,
                     "[k_wf_mesh] rays %llu  node code: %llu wave iterations, %.1f %% lanes active;  triangle code: %llu, %.1f %%;  "
                     "refill: %llu, %.1f %%;  stack entries culled on pop %llu\n",
                     hc.mesh_rays, hc.node_wave_iters, pct(hc.node_visits, hc.node_wave_iters), hc.tri_wave_iters,
                     pct(hc.tri_tests, hc.tri_wave_iters), hc.refill_wave_iters, pct(hc.refill_lanes, hc.refill_wave_iters), hc.pops_culled);
    }
    st.pipeline_used = RT_PIPELINE_WAVEFRONT;
    st.samples = samples;
    st.rays = hc.rays;
    st.mesh_rays = hc.mesh_rays;
    st.node_visits = hc.node_visits;
    st.tri_tests = hc.tri_tests;
    st.prim_tests = hc.prim_tests;
    st.bytes_node = su.split ? (su.node_kind == 0 ? sizeof(BvhNode4f) : sizeof(BvhNode4q)) : sizeof(BvhNode<R>);
    st.bytes_tri = sizeof(TriRec<R>);
    st.bytes_attr = sizeof(TriAttr<R>);
    // path state moved by the DOMINANT kernel per ray it traverses: ray (6 R) + bound/op read (R + 4)
    // + hit written when a triangle wins (3 R + 8) + queue entry (4)
    st.bytes_state = 6 * sizeof(R) + sizeof(R) + 4 + 3 * sizeof(R) + 8 + 4;
    // k_wf_prims per ray: ray in (6 R), closest hit out (3 R + 8); k_wf_shade per ray: ray + hit + throughput + rng + depth +
    // sample index in, ray + throughput + rng + depth out (a path that ends writes 24 B of radiance instead and restarts)
    st.bytes_state_prims = 6 * sizeof(R) + 3 * sizeof(R) + 8;
    st.bytes_state_shade = (6 + 3 + 3) * sizeof(R) + 8 + 8 + 4 + 8 + (6 + 3) * sizeof(R) + 8 + 4;
    // the lean renders of this scene run the search inside k_wf_shade: its bytes per ray are then the kernel's (a counting
    // render is never fused, but it reports what the timed renders beside it move)
    if (fusable) st.bytes_state_shade += st.bytes_state_prims;
    if (!su.split) st.mesh_rays = hc.rays;  // combined kernel: every ray's state passes through it
    return RT_OK;
}

// What a call of render_wavefront settles before its first replica group, whatever its mode: the pool's size, the replicas per
// group, the search setup, the LDS forms of k_wf_shade and the environment switches of the loop.
template <typename R>
struct WfRun {
    SearchSetup<R> su;
    uint32_t capacity, group, staged_shade, shade_tables_max, compact_min, compact_pct, check_every, shade_lds_pad;
    int lds_shade;
    bool tex, compact_tail, iter_log, trace_pool, fusable;  // fusable: the scene and the switches allow the fused k_wf_shade; the mode's group type has the other say
    template <typename G> ShadeKernel<R, G> shade(bool fuse) const { return pick_shade<R, G>(su.stats, lds_shade, tex, fuse); }
};

// npix_frame, T: the whole frame's, for the pool; the rest describes this call's samples (wf_plan_samples).
template <typename R>
int wf_prepare(RtScene* s, DeviceScene<R>& ds, const RtRenderParams& p, uint64_t npix_frame, uint64_t npix, uint32_t n, uint32_t sample_bytes,
               bool running_sums, WfRun<R>& run) {
    const uint32_t strata = p.sqrt_spt * p.sqrt_spt;
    uint32_t capacity = wf_pool_capacity(strata, npix_frame, p.thread_count);
    // the pool is a matter of speed, not of correctness: when device memory is short (other scenes of a frame pipeline, other
    // processes on the card) a smaller one renders the same frame
    for (;;) {
        const int st = wf_ensure<R>(s, capacity);
        if (st == RT_OK) break;
        if (st != RT_E_NOMEM || capacity <= (1u << 20) || std::getenv("RT_WF_POOL")) return st;
        capacity = std::max<uint32_t>(1u << 20, (capacity / 2) & ~0xFFFFFu);
    }
    run.capacity = capacity;
    if (int st = wf_plan_samples(s->wf, uint64_t(strata) * npix, npix, n, sample_bytes, running_sums, &run.group)) return st;
    const bool vol = !s->compiled.volumes.empty();  // volume ops: combined intersect kernel, VOL variant
    SearchSetup<R>& su = run.su;
    if (int st = make_search_setup<R>(s, ds, p.collect_stats != 0, vol, &su)) return st;
    if (int st = s->wf.mesh_spill.reserve(su.spill_bytes)) return st;
    run.staged_shade = staged_prefix(ds.view.lay_shade, su.lds_tables, su.lds_budget);
    // k_wf_shade: all or nothing (a staged prefix read through flat instructions was 3 % slower than global memory on the default scene),
    // and only while five workgroups still fit a CU's 160 KB next to its lists (<= 23 KB of tables; RT_LDS_SHADE_MAX overrides)
    run.shade_tables_max = env_u32("RT_LDS_SHADE_MAX", 32u * 1024u - kShadeListBytes);
    run.lds_shade = (run.staged_shade != 0 && run.staged_shade == ds.view.lay_shade.total_bytes && run.staged_shade <= run.shade_tables_max) ? 1 : (env_u32("RT_LDS_SHADE_PREFIX", 0) && run.staged_shade ? 2 : 0);
    // tail compaction: RT_WF_COMPACT=0 keeps the paths where they are (A/B, tests), RT_WF_COMPACT_MIN = fewest paths worth a launch
    run.compact_tail = env_u32("RT_WF_COMPACT", 1) != 0;
    run.compact_min = std::max<uint32_t>(1u, env_u32("RT_WF_COMPACT_MIN", 1024));
    run.compact_pct = std::min<uint32_t>(75u, std::max<uint32_t>(1u, env_u32("RT_WF_COMPACT_PCT", 50)));  // ... when at most this share of the addressed slots is alive.  50 / 62 / 75: the tail's iterations of C2 take 13.0 / 12.4 / 11.9 ms, but the paths thin out by ~22 % per iteration, so 75 compacts after nearly every one (13 copies of 0.3 ms per C2 frame, 6 with 50); whole frames are equal within the noise
    run.iter_log = env_u32("RT_WF_ITER_LOG", 0) != 0;
    run.trace_pool = env_u32("RT_WF_TRACE", 0) != 0;  // debug: dump the first pool slots after every iteration
    run.check_every = run.trace_pool ? 1u : std::min<uint32_t>(32u, std::max<uint32_t>(1u, env_u32("RT_WF_CHECK", 8)));  // 4 timing events per iteration, 128 events
    run.tex = s->compiled.needs_tex_interpreter;
    run.shade_lds_pad = env_u32("RT_WF_SHADE_LDS_PAD", 0);  // experiments: fewer resident blocks of the shade kernel
    // k_wf_prims as phase 4 of k_wf_shade (rt_wavefront.h): the lean dense variant with BOTH table sets staged whole in LDS, the
    // prims set within what the shade kernel may ask for at five workgroups per CU.  With the tables in global memory the fused
    // kernel needs scratch (f64 32 B, f32 80 B; tools/kernel_regs.py), so those scenes - and volumes, re-built groups, the texture
    // interpreter and the counting variants - keep the stand-alone kernel; so do the group types without a fused kernel
    // (kShadeFused: sparse adaptive passes, light-group renders), which is the caller's to add.
    // Programs with more than one mesh op keep it too: tests/scenes/two_meshes lost 2.4 % of its frame fused (DESIGN.md section 6,
    // round 5).  RT_WF_FUSE=0: the unfused pipeline (A/B control, reference of the tests); 2: fused wherever the kernel exists,
    // whatever the plan says (tests, A/B).
    const uint32_t fuse_mode = env_u32("RT_WF_FUSE", 1);
    run.fusable = (su.split || su.prims_only) && !vol && !su.groups && !run.tex && su.lds_prims == 1 && run.lds_shade == 1 &&
                  su.staged_prims <= run.shade_tables_max && fuse_mode != 0 && (!su.plan.multi_mesh || fuse_mode == 2);
    // Every kernel the modes instantiate for R, named once, behind the search kernels.  The compiler emits a kernel where it is
    // first named, so this list - in the order the code object has had since the driver was one function that named them all -
    // keeps the library's device code byte for byte the same whichever mode's driver is instantiated first
    // (profiles/wavefront_modes/README.md); WfRun::shade, not pick_shade itself, is what the driver calls for the same reason.
    (void)&pick_shade<R, WfGroup<R>>, (void)&pick_shade<R, WfGroupSparse<R>>, (void)&pick_shade<R, WfGroupLG<R>>;
    (void)&pick_shade<R, WfGroupRays<R>>, (void)&pick_shade<R, WfGroupPoints<R>>;
    (void)&pick_shade<R, WfGroupProbes<R>>;
    (void)&k_wf_generate<R, WfGroupPoints<R>>, (void)&k_wf_generate<R, WfGroupRays<R>>, (void)&k_wf_generate<R, WfGroupSparse<R>>, (void)&k_wf_generate<R, WfGroup<R>>;
    (void)&k_wf_compact<R>, (void)&k_wf_resolve_moments<true>, (void)&k_wf_resolve_moments<false>;
    (void)&k_wf_generate<R, WfGroupProbes<R>>, (void)&k_wf_resolve_sh<R>;
    return RT_OK;
}

// One replica group through the pool: k_wf_generate, then search and k_wf_shade until the queue is empty, tail compaction
// included.  The group type G is all this knows of the call's mode: G's generate kernel, and the k_wf_shade picked for G.
template <typename R, typename G>
int wf_run_group(RtScene* s, DeviceScene<R>& ds, const WfRun<R>& run, const G& grp, ShadeKernel<R, G> shade, bool fuse, const CameraView<R>& cv,
                 const ParamsView<R>& pv, bool last_group, hipStream_t stream, WfTally& ty) {
    RtScene::Wavefront& w = s->wf;
    const SearchSetup<R>& su = run.su;
    const PoolPair<R>& pools = std::get<PoolPair<R>>(w.pools);
    const WfPool<R> pool_a = pools[0].view, pool_b = pools[1].view;
    WfPool<R> pool = pool_a;  // the pool the kernels are working on (changes at a tail compaction)
    const WfPool<R>* pool_dev_cur = pools[0].dev;
    uint32_t* const queue[2] = {pools[0].queue[0], pools[0].queue[1]};
    uint32_t* const mesh_queue = pools[0].mesh_queue;
    const size_t shade_tables_lds = run.lds_shade == 0 ? size_t(0) : (fuse ? size_t(std::max(run.staged_shade, su.staged_prims)) : size_t(run.staged_shade));
    bool prims_ran[32];  // per iteration of a batch (check_every <= 32): k_wf_prims was launched
    uint32_t first = uint32_t(std::min<uint64_t>(run.capacity, grp.total));
    bool on_b = false;
    pool.capacity = first;  // slots in use by this group: the kernels address slots directly while all of them are queued
    *w.h_ctr = WfCounters{first, 0, 0, 0, first, 0};  // n_in, n_out, cursor, n_mesh, next_sample, n_mesh_next
    HIP_TRY(hipMemcpyAsync(w.d_ctr, w.h_ctr, sizeof(WfCounters), hipMemcpyHostToDevice, stream));
    // k_wf_generate is the group type's own wherever the group's first rays are (active list, ray table, point table); a
    // light-group render starts its samples as a plain frame does, through WfGroup's kernel: no instantiation of its own
    hipLaunchKernelGGL((k_wf_generate<R, std::conditional_t<G::kLightGroups, WfGroup<R>, G>>), dim3((first + 255) / 256), dim3(256), 0, stream, pool, first, grp, cv, pv, queue[0]);
    int qi = 0;
    bool hits_ready = false;  // the hit records and the mesh queue of the current queue exist already (phase 4 of a fused k_wf_shade)
    uint32_t upper = first;  // upper bound of the queue length (never grows: slots are reused in place)
    for (;;) {
        size_t ev = 0;
        // near the end of the call's last group the host looks after every second iteration, so that the tail is seen when it starts
        const bool near_end = s->tail_flag && last_group && w.h_ctr->next_sample + 4ull * pool.capacity >= grp.total;
        // tail compaction wants to see the queue length of every iteration once the samples have run out, and to notice
        // within two iterations that they have (a quarter of the slots restarts per iteration)
        const bool all_started = w.h_ctr->next_sample >= grp.total;
        const bool closing = run.compact_tail && w.h_ctr->next_sample + 2ull * pool.capacity >= grp.total;
        const uint32_t check_now = (run.compact_tail && all_started) ? 1u : ((near_end || closing) ? std::min<uint32_t>(run.check_every, 2u) : run.check_every);
        for (uint32_t k = 0; k < check_now; k++) {
            HIP_TRY(hipEventRecord(w.events[ev++], stream));
            const SearchQueues sq{queue[qi], mesh_queue, w.mesh_spill, w.d_ctr, s->d_counters, stream};
            prims_ran[k] = (su.split || su.prims_only) && !hits_ready;
            if (prims_ran[k]) launch_prims(su, ds, pool, sq, upper);
            HIP_TRY(hipEventRecord(w.events[ev++], stream));
            if (su.split) launch_mesh(su, ds, pool, sq);
            else if (!su.prims_only) launch_intersect(su, ds, pool, sq);  // the combined kernel
            if (prims_ran[k] || !(su.split || su.prims_only)) ty.search_launches++;
            HIP_TRY(hipEventRecord(w.events[ev++], stream));
            hipLaunchKernelGGL(shade, dim3((upper + WF_CHUNK - 1) / WF_CHUNK), dim3(256), shade_tables_lds + kShadeListBytes + run.shade_lds_pad, stream,
                               ds.view, cv, pv, pool, grp, queue[qi], queue[qi ^ 1], w.d_ctr.get(), w.sample_L.get(), s->d_counters.get(),
                               pool_dev_cur, run.staged_shade, mesh_queue);
            if (fuse) hits_ready = true;  // + k_wf_prims' search for the next queue: the next iteration starts at k_wf_mesh
            hipLaunchKernelGGL(k_wf_advance, dim3(1), dim3(1), 0, stream, w.d_ctr.get());
            HIP_TRY(hipEventRecord(w.events[ev++], stream));
            qi ^= 1;
            ty.iterations++;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.h_ctr, w.d_ctr, sizeof(WfCounters), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (size_t e = 0; e + 3 < ev; e += 4) {
            float it_ms[3];
            for (int ph = 0; ph < 3; ph++) {
                it_ms[ph] = 0.f;
                HIP_TRY(hipEventElapsedTime(&it_ms[ph], w.events[e + ph], w.events[e + ph + 1]));
                if (ph == 0 && (su.split || su.prims_only) && !prims_ran[e / 4]) it_ms[ph] = 0.f;  // no launch between the two events
                ty.phase_ms[ph] += it_ms[ph];
            }
            if (run.iter_log)  // RT_WF_ITER_LOG=1 (with RT_WF_CHECK=1 the queue length printed is the one of this very iteration)
                std::fprintf(stderr, "[wf iter] group %u: <= %u paths queued: prims %.3f ms, traversal %.3f ms, shade %.3f ms\n", ty.n_groups, upper,
                             it_ms[0], it_ms[1], it_ms[2]);
        }
        if (run.trace_pool)
            if (int st = wf_trace_dump(pool, first, queue[qi], w.h_ctr->n_in, ty.iterations)) return st;
        upper = w.h_ctr->n_in;
        // every sample of the call's last group has been started and slots are running empty: from here on this render
        // cannot fill the GPU any more, the next frame's render (another RtScene, another stream) may start underneath it
        if (s->tail_flag && last_group && upper < first) __atomic_store_n(s->tail_flag, 1, __ATOMIC_RELEASE);
        if (upper == 0) break;
        // ---- tail compaction (rt_wavefront.h k_wf_compact): fewer than half of the addressed slots are alive and none will
        //      restart: the live paths move to slots 0 .. upper-1 of the other pool, which becomes the pool ----
        if (run.compact_tail && w.h_ctr->next_sample >= grp.total && upper >= run.compact_min && uint64_t(upper) * 100 <= uint64_t(pool.capacity) * run.compact_pct) {
            WfPool<R> dst = on_b ? pool_a : pool_b;
            hipLaunchKernelGGL((k_wf_compact<R>), dim3((upper + 255) / 256), dim3(256), 0, stream, pool, dst, queue[qi], upper);
            on_b = !on_b;
            pool = dst;
            pool.capacity = upper;  // n_in == capacity: the kernels address slot i for entry i again
            pool_dev_cur = pools[on_b ? 1 : 0].dev;
            ty.n_compactions++;
            if (hits_ready) {  // the hit records stayed behind and the mesh queue names the old slots: stand-alone k_wf_prims next
                HIP_TRY(hipMemsetAsync(&w.d_ctr->n_mesh, 0, sizeof(uint32_t), stream));
                hits_ready = false;
            }
        }
    }
    return RT_OK;
}

template <typename R, typename Pass>
int render_wavefront(RtScene* s, DeviceScene<R>& ds, const RtCameraDesc& cam, const RtRenderParams& p, uint32_t owned,
                     uint32_t t_first, uint32_t n, double* d_out, hipStream_t stream, const Pass& pass) {
    using G = typename Pass::template Group<R>;
    CameraView<R> cv = make_camera_view<R>(cam, p);
    if (Pass::kOwnOrigins) cv.has_aperture = 1;  // k_wf_shade's restarts store the origin (phase 2)
    ParamsView<R> pv = make_params_view<R>(p, owned);
    const uint64_t npix_frame = uint64_t(cam.image_width) * owned;
    const uint64_t npix = pass.npix(npix_frame);  // pixels a replica group covers
    if (Pass::kNoCounting && p.collect_stats) return set_err(RT_E_UNSUPPORTED, Pass::kNoCounting);
    if (npix == 0) return set_err(RT_E_INVALID, "adaptive pass without active pixels");
    const uint32_t strata = p.sqrt_spt * p.sqrt_spt;
    const uint32_t t_end = t_first + n;
    const uint64_t per_replica = uint64_t(strata) * npix;
    WfRun<R> run;
    if (int st = wf_prepare<R>(s, ds, p, npix_frame, npix, n, Pass::kSampleBytes, Pass::kRunningSums, run)) return st;
    if (int st = pass.reserve(s->wf, per_replica, npix, run.group, n, stream)) return st;
    const bool fusable = run.fusable && kShadeFused<G>;
    const bool fuse = fusable && !run.su.stats;
    const ShadeKernel<R, G> shade = run.template shade<G>(fuse);

    HIP_TRY(hipMemsetAsync(s->d_counters, 0, sizeof(DeviceCounters), stream));
    HIP_TRY(hipEventRecord(s->ev0, stream));
    WfTally ty{};
    for (uint32_t t0 = t_first; t0 < t_end; t0 += run.group) {
        ty.n_groups++;
        const uint32_t nrep = std::min(run.group, t_end - t0);
        const bool last_group = t0 + nrep >= t_end;
        G grp{};  // the base: total, npix, per_replica, their reciprocals and the width's, tid0, strata; the rest is the mode's
        static_cast<WfGroup<R>&>(grp) = WfGroup<R>{per_replica * nrep, npix, per_replica, 1.0 / double(per_replica), 1.0 / double(npix), 1.0 / double(cam.image_width), t0, strata};
        pass.complete(grp, s->wf);
        if (grp.total >= (1ull << 51)) return set_err(RT_E_UNSUPPORTED, "more than 2^51 samples in one replica group");
        if (int st = wf_run_group(s, ds, run, grp, shade, fuse, cv, pv, last_group, stream, ty)) return st;
        if (int st = pass.resolve(WfResolve{s->wf, npix, strata, nrep, p.thread_count, t0, pv.spp, d_out, int(t0 == t_first), int(t_first > 0), int(last_group), stream})) return st;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
#ifdef RT_SHADE_STAMPS
    {
        unsigned long long h[16];
        HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_shade_stamps), sizeof h));
        const double trips = double(h[8] ? h[8] : 1);
        const char* names[7] = {"loop head / previous trip's tail", "state loads + resolve_hit", "throughput / rng loads + shade_hit", "stores + list appends",
                                "barrier after phase 1", "phase 2 (restarts)", "barrier + phase 3 (queue)"};
        std::fprintf(stderr, "[k_wf_shade stamps] %llu waves, %llu wave-trips (cumulative over the process)\n", h[9], h[8]);
        for (int k = 0; k < 7; k++) std::fprintf(stderr, "  %-40s %10.0f clk per wave-trip\n", names[k], double(h[k]) / trips);
    }
#endif
    return wf_fill_stats(s, run.su, ty, fusable, npix * strata * n);
}

// ---------------------------------------------------------------------------------------------
// The search pass of a ray query (the query itself: rt_query.hip)
// ---------------------------------------------------------------------------------------------
// One pass of the scene's search kernels over slots 0 .. m-1 of the query pool: what render_wavefront launches at the head
// of an iteration of a lean (no counters), volume-free render, from the same make_search_setup and through the same launch
// helpers, with the query workspace's queues, counters and spill buffer.
template <typename R>
int query_search_pass(RtScene* s, DeviceScene<R>& ds, const PathPool<R>& pl, uint32_t m, hipStream_t stream) {
    RtScene::Query& q = s->rq;
    SearchSetup<R> su;
    if (int st = make_search_setup<R>(s, ds, false, false, &su)) return st;
    if (int st = q.mesh_spill.reserve(su.spill_bytes)) return st;
    WfPool<R> pool = pl.view;
    pool.capacity = m;  // every slot is queued: the kernels address slot i for entry i
    WfCounters init{};
    init.n_in = m;
    *q.h_ctr = init;
    HIP_TRY(hipMemcpyAsync(q.d_ctr, q.h_ctr, sizeof(WfCounters), hipMemcpyHostToDevice, stream));
    const SearchQueues sq{pl.queue[0], pl.mesh_queue, q.mesh_spill, q.d_ctr, s->d_counters, stream};
    if (su.split || su.prims_only) {
        launch_prims(su, ds, pool, sq, m);
        if (su.split) launch_mesh(su, ds, pool, sq);
    } else {
        launch_intersect(su, ds, pool, sq);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// Renders along ray tables (include/rt_mi355.h)
// ---------------------------------------------------------------------------------------------
// Rays (or bake points) per chunk.  A chunk is rendered like a frame of that many pixels (pool, per-sample buffer, replica groups), so the
// default is a frame's order of magnitude, 2^22 = a 2048 x 2048 image; it is a guess, not a measurement.  At most 2^28: the
// kernels index the table with 32-bit element offsets.
static uint32_t rays_chunk() { return std::min<uint32_t>(1u << 28, std::max<uint32_t>(1u, env_u32("RT_RAYS_CHUNK", 1u << 22))); }

void stats_add(RtRenderStats& total, const RtRenderStats& part, bool first) {
    if (first) { total = part; return; }
    total.kernel_ms += part.kernel_ms; total.traversal_kernel_ms += part.traversal_kernel_ms;
    total.prims_kernel_ms += part.prims_kernel_ms; total.shade_kernel_ms += part.shade_kernel_ms;
    total.n_launches += part.n_launches; total.n_iterations += part.n_iterations; total.samples += part.samples;
    total.n_replica_groups += part.n_replica_groups; total.n_tail_compactions += part.n_tail_compactions;
}

// n table entries (rays, points, probes) in chunks through render_wavefront, each chunk a frame of m x 1 pixels whose pixel i is
// entry off + i: make_pass(p, off, m, d_in) is the chunk's pass (d_in: the chunk's part of each array of `in`, on the device), and
// after(off, m, d_out, stream) may enqueue more work on the chunk's output.  host: the arrays are the caller's host memory and go through
// the staging buffer.  The scene's stats are the sums over the chunks; the tail flag belongs to the last chunk.
struct NoAfter {
    int operator()(uint64_t, uint32_t, double*, hipStream_t) const { return RT_OK; }
};
template <typename R, typename MakePass, typename After>
int render_table_chunks(RtScene* s, DeviceScene<R>& ds, const RtRenderParams& p, uint64_t n, const std::vector<ChunkArray>& in, double* out, size_t out_each,
                        bool host, hipStream_t stream, MakePass&& make_pass, After&& after) {
    RtCameraDesc cam{};  // only the width is read: a table has no camera arithmetic
    cam.image_height = 1;
    RtRenderStats sum{};
    int32_t* const tail_flag = s->tail_flag;
    ChunkTimes t;
    auto launch = [&](uint64_t off, uint32_t m, const void* const* d_in, void* d_out) -> int {
        cam.image_width = m;
        s->tail_flag = off + m >= n ? tail_flag : nullptr;
        const int st = render_wavefront(s, ds, cam, p, 1u, 0u, p.thread_count, static_cast<double*>(d_out), stream, make_pass(p, off, m, d_in));
        s->tail_flag = tail_flag;
        if (st != RT_OK) return st;
        stats_add(sum, s->stats, off == 0);
        return after(off, m, static_cast<double*>(d_out), stream);
    };
    const int st = run_chunks(s->rays.stage, n, rays_chunk(), host, in, out, out_each, stream, launch, &t);
    if (st == RT_OK) s->stats = sum;
    return st;
}

// The three table modes: what fills a chunk's pass from the call's parameters and the chunk's arrays on the device.
static RayTablePass ray_table_pass(const RtRenderParams&, uint64_t off, uint32_t, const void* const* d_in) {
    RayTablePass rp;
    rp.first = off;
    rp.origins = static_cast<const double*>(d_in[0]);
    rp.dirs = static_cast<const double*>(d_in[1]);
    return rp;
}
// HITS: d_in[0] is the chunk's first RtRayHit record; else d_in[0] / d_in[1] are its first position / normal.
template <bool HITS>
PointTablePass point_table_pass(const RtRenderParams&, uint64_t off, uint32_t, const void* const* d_in) {
    const HitPoints h = HITS ? hit_points(static_cast<const RtRayHit*>(d_in[0]))
                             : HitPoints{static_cast<const unsigned char*>(d_in[0]), static_cast<const unsigned char*>(d_in[1]), nullptr, 24u};
    PointTablePass pp;
    pp.first = off;
    pp.pos = h.pos;
    pp.nrm = h.nrm;
    pp.stride = h.stride;
    return pp;
}
// Records without a surface point are zeroed after the chunk's resolve.
static int points_mask(const RtRayHit* hits, uint32_t m, double* d_out, hipStream_t stream) {
    const HitPoints h = hit_points(hits);
    hipLaunchKernelGGL(k_wf_points_mask, dim3((m + 255) / 256), dim3(256), 0, stream, h.flags, h.stride, m, d_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
static ProbeTablePass probe_table_pass(const RtRenderParams& p, uint64_t off, uint32_t, const void* const* d_in) {
    ProbeTablePass pp;
    pp.first = off;
    pp.pos = static_cast<const double*>(d_in[0]);
    pp.seed = p.seed;
    pp.S = p.sqrt_spt;
    pp.f32 = p.precision == RT_PRECISION_F32;
    return pp;
}

// ---------------------------------------------------------------------------------------------
// Table modes: the entry points of ray tables, irradiance and probe bakes
// ---------------------------------------------------------------------------------------------
// The rules the table modes share, checked before the device is touched; a call's description (TableCall) is in
// rt_scene_host.h, because rt_bake_lightmap runs these rules too.
int table_render_check(const RtScene* scene, uint64_t n, const RtRenderParams* params, const void* out, const TableCall& c) {
    const std::string w = std::string(c.who) + ": ";
    if (!scene) return set_err(RT_E_INVALID, w + "scene is NULL");
    if (!params) return set_err(RT_E_INVALID, w + "params is NULL");
    if (params->sqrt_spt == 0) return set_err(RT_E_INVALID, w + "sqrt_spt must be positive");
    if (params->thread_count == 0) return set_err(RT_E_INVALID, w + "thread_count must be positive");
    if (params->precision != RT_PRECISION_F64 && params->precision != RT_PRECISION_F32) return set_err(RT_E_INVALID, w + "precision must be RT_PRECISION_F64 or RT_PRECISION_F32");
    if (params->n_parts > 1) return set_err(RT_E_INVALID, w + "n_parts > 1: a " + c.what + " has no row partition");
    if (n >= (1ull << 31)) return set_err(RT_E_INVALID, w + "n must be below 2^31");
    if (uint64_t(params->sqrt_spt) * params->sqrt_spt * params->thread_count > 0xFFFFFFFFull) return set_err(RT_E_UNSUPPORTED, w + "more than 2^32 samples per " + c.unit + " (sqrt_spt, thread_count)");
    if (params->pipeline == RT_PIPELINE_MEGAKERNEL) return set_err(RT_E_UNSUPPORTED, w + c.what + "s run the wavefront scheduler: pipeline = RT_PIPELINE_MEGAKERNEL is not supported");
    if (params->pipeline != RT_PIPELINE_AUTO && params->pipeline != RT_PIPELINE_WAVEFRONT) return set_err(RT_E_INVALID, w + "unknown pipeline");
    if (params->max_depth == 0) return set_err(RT_E_UNSUPPORTED, w + "max_depth = 0 is not supported");
    if (params->collect_stats) return set_err(RT_E_UNSUPPORTED, w + c.what + "s have no counting kernels (collect_stats)");
    if (n == 0) return RT_OK;
    for (const TableArray* t : {&c.a, &c.b})
        if (t->name && !t->p) return set_err(RT_E_INVALID, w + t->name + " is NULL");
    if (!out) return set_err(RT_E_INVALID, w + c.out_name + " is NULL");
    return RT_OK;
}

// The checks, the scene's tables in params->precision, then the chunks (render_table_chunks has make_pass and after).  Whoever
// waits for this render's tail (rt_scene_set_tail_flag) is released at the latest here, errors and early returns included.
template <typename MakePass, typename After = NoAfter>
int table_call(const RtScene* scene, uint64_t n, const RtRenderParams* params, double* out, bool host, void* stream, const TableCall& c,
               MakePass&& make_pass, After&& after = After{}) {
    const int r = [&]() -> int {
        if (int st = table_render_check(scene, n, params, out, c)) return st;
        if (n == 0) return RT_OK;
        RtScene* s = const_cast<RtScene*>(scene);  // workspace + lazily built tables; the scene data itself is immutable
        HIP_TRY(hipSetDevice(s->device));
        RtRenderParams p = *params;
        p.band_rows = p.n_parts = p.part = 0;
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
        std::vector<ChunkArray> in;
        for (const TableArray* t : {&c.a, &c.b})
            if (t->name) in.push_back({t->p, t->each});
        return with_tables(s, p.precision, [&](auto& ds) -> int { return render_table_chunks(s, ds, p, n, in, out, c.out_each, host, st, make_pass, after); });
    }();
    if (scene && scene->tail_flag) __atomic_store_n(scene->tail_flag, 1, __ATOMIC_RELEASE);
    return r;
}

// A device buffer of `bytes` for the length of one call of a host variant: run(d) works on it, then (on success) `bytes_back`
// bytes from its start go to `host_out`.
template <typename F>
int with_device_frame(size_t bytes, void* host_out, size_t bytes_back, F&& run) {
    DevBuf<double> d;
    if (int st = d.reserve(bytes)) return st;
    if (int st = run(d.get())) return st;
    const hipError_t e = hipMemcpy(host_out, d, bytes_back, hipMemcpyDeviceToHost);
    return e == hipSuccess ? int(RT_OK) : set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
}

int validate_render_args(const RtCameraDesc* camera, const RtRenderParams* params) {
    if (params->sqrt_spt == 0 || params->thread_count == 0) return set_err(RT_E_INVALID, "sqrt_spt and thread_count must be positive");
    if (params->band_rows != 0 && params->n_parts > 1 && params->part >= params->n_parts) return set_err(RT_E_INVALID, "part >= n_parts");
    if (camera->image_width == 0 || camera->image_height == 0) return set_err(RT_E_INVALID, "empty image");
    if (uint64_t(params->sqrt_spt) * params->sqrt_spt * params->thread_count > 0xFFFFFFFFull)
        return set_err(RT_E_UNSUPPORTED, "more than 2^32 samples per pixel");
    if (params->precision != RT_PRECISION_F64 && params->precision != RT_PRECISION_F32) return set_err(RT_E_INVALID, "unknown precision");
    return RT_OK;
}

}  // namespace rt

// Probe of fuzzy_reflection (rt_device.h): the routine with its fuzz == 0 shortcut next to the plain expression of
// metal.rs:33-35 / glossy.rs:66-68, same inputs, same generator state (tests/test_gpu_parity.py).
namespace rt {
__global__ void k_debug_fuzzy_reflection(uint32_t n, const double* __restrict__ reflected, const double* __restrict__ fuzz,
                                         const unsigned long long* __restrict__ state, double* __restrict__ out, unsigned long long* __restrict__ state_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3<double> r = mk<double>(reflected[3 * i], reflected[3 * i + 1], reflected[3 * i + 2]);
    Rng a, b;
    a.s = b.s = state[i];
    const V3<double> da = fuzzy_reflection(r, fuzz[i], a);
    const V3<double> db = r + random_unit<double>(b) * fuzz[i] * length(r);
    out[6 * i + 0] = da.x; out[6 * i + 1] = da.y; out[6 * i + 2] = da.z;
    out[6 * i + 3] = db.x; out[6 * i + 4] = db.y; out[6 * i + 5] = db.z;
    state_out[2 * i] = a.s; state_out[2 * i + 1] = b.s;
}
}  // namespace rt

namespace rt {
// The mesh export (rt_desc.h) from the tables a scene holds on the device
template <typename R>
static int mesh_export_device(const CompiledScene& cs, const CompiledScene::MeshGeom& g, const DeviceScene<R>& ds, const MeshExportOut& o) {
    std::vector<MeshNode4qc> nodes(g.n_nodes4);
    std::vector<TriRec<R>> tris(g.n_tris);
    if (g.n_nodes4) HIP_TRY(hipMemcpy(nodes.data(), ds.view.nodes4q + g.node4_base, nodes.size() * sizeof(MeshNode4qc), hipMemcpyDeviceToHost));
    if (g.n_tris) HIP_TRY(hipMemcpy(tris.data(), ds.view.tris + g.tri_base, tris.size() * sizeof(TriRec<R>), hipMemcpyDeviceToHost));
    mesh_export<R>(g, nodes.data(), tris.data(), cs.tri_order.data() + g.tri_base, o);
    return RT_OK;
}

// The refit kernels of one arithmetic type over every moved mesh, enqueued on the scene's stream; `ds` holds the mesh tables.
template <typename R>
static int refit_typed(RtScene* s, const CompiledScene& cs, const std::vector<uint32_t>& moved, DeviceScene<R>& ds) {
    for (uint32_t gi : moved) {
        const CompiledScene::MeshGeom& g = cs.mesh_geoms[gi];
        RefitTarget<R> t{};
        t.nodes = const_cast<BvhNode<R>*>(ds.view.nodes) + g.node_base;
        t.nodes4 = const_cast<BvhNode4f*>(ds.view.nodes4) + g.node4_base;
        t.nodes4q = const_cast<MeshNode4qc*>(ds.view.nodes4q) + g.node4_base;
        t.tris = const_cast<TriRec<R>*>(ds.view.tris) + g.tri_base;
        t.attrs = const_cast<TriAttr<R>*>(ds.view.attrs) + g.tri_base;
        t.pad4 = mesh_pad(cs, g);
        std::string err;
        if (!refit_mesh_launch<R>(s->refit[gi], t, s->stream, &err)) return set_err(RT_E_DEVICE, err);
    }
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// What a client of the renderer uses (rt_render.h; the accumulator in rt_accum.hip)
// ---------------------------------------------------------------------------------------------
int render_replicas(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                    uint32_t t_first, uint32_t n, double* d_rgba_out, void* stream, const AdaptivePass* ad) {
    if (!scene || !camera || !params || !d_rgba_out) return set_err(RT_E_INVALID, "rt_render_device: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    if (n == 0 || t_first + uint64_t(n) > params->thread_count) return set_err(RT_E_INVALID, "replica range outside [0, thread_count)");
    RtScene* s = const_cast<RtScene*>(scene);  // stats + lazily built tables; the scene data itself is immutable
    HIP_TRY(hipSetDevice(s->device));
    uint32_t owned = owned_rows(camera->image_height, params);
    if (owned == 0) return RT_OK;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
    // AUTO: the wavefront scheduler (since its state accesses are coalesced streams it beats the per-pixel
    // megakernel on every scene measured, with or without meshes); RT_AUTO_MEGA_NO_MESH=1 restores the old rule
    bool has_mesh = !s->compiled.meshes.empty();
    bool wavefront = params->pipeline == RT_PIPELINE_WAVEFRONT ||
                     (params->pipeline == RT_PIPELINE_AUTO && (has_mesh || env_u32("RT_AUTO_MEGA_NO_MESH", 0) == 0));
    if (params->max_depth == 0) wavefront = false;  // every sample is black (camera.rs:290): nothing to schedule
    if (ad) {  // adaptive passes exist in the wavefront scheduler only
        if (params->pipeline == RT_PIPELINE_MEGAKERNEL) return set_err(RT_E_UNSUPPORTED, "adaptive passes run the wavefront scheduler: RT_PIPELINE_MEGAKERNEL is not supported");
        if (params->max_depth == 0) return set_err(RT_E_UNSUPPORTED, "adaptive sampling with max_depth = 0");
        wavefront = true;  // collect_stats: refused by the mode
    }
    return with_tables(s, params->precision, [&](auto& ds) -> int {
        if (ad && ad->sparse) return render_wavefront(s, ds, *camera, *params, owned, t_first, n, d_rgba_out, st, AdaptiveMode<true>{*ad});
        if (ad) return render_wavefront(s, ds, *camera, *params, owned, t_first, n, d_rgba_out, st, AdaptiveMode<false>{*ad});
        if (wavefront) return render_wavefront(s, ds, *camera, *params, owned, t_first, n, d_rgba_out, st, FramePass{});
        return render_typed(s, ds, *camera, *params, owned, t_first, n, d_rgba_out, st);
    });
}

int render_aov_replicas(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                        double* d_out, void* stream) {
    if (!scene || !camera || !params || !d_out) return set_err(RT_E_INVALID, "rt_render_aov: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    if (n_replicas == 0 || n_replicas > params->thread_count) return set_err(RT_E_INVALID, "rt_render_aov: n_replicas must be in 1 .. thread_count");
    RtScene* s = const_cast<RtScene*>(scene);  // lazily built tables only
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t owned = owned_rows(camera->image_height, params);
    if (owned == 0) return RT_OK;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
    return with_tables(s, params->precision, [&](auto& ds) { return aov_typed(s, ds, *camera, *params, owned, n_replicas, d_out, st); });
}

int scene_device(const RtScene* s) { return s->device; }
hipStream_t scene_stream(const RtScene* s) { return s->stream; }
uint64_t scene_generation(const RtScene* s) { return s->generation; }
uint64_t scene_content_digest(const RtScene* s) { return s->content_digest; }
const RtRenderStats& scene_stats(const RtScene* s) { return s->stats; }
void scene_set_stats(RtScene* s, const RtRenderStats& stats) { s->stats = stats; }
int32_t* scene_tail_flag(const RtScene* s) { return s->tail_flag; }
void scene_set_tail_flag(RtScene* s, int32_t* flag) { s->tail_flag = flag; }
void scene_release_tail(const RtScene* s) {
    if (s->tail_flag) __atomic_store_n(s->tail_flag, 1, __ATOMIC_RELEASE);
}
}  // namespace rt

extern "C" {

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_scene_create(const RtSceneDesc* desc, int device, RtScene** out) {
    using namespace rt;
    if (!out) return set_err(RT_E_INVALID, "rt_scene_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<RtScene> s(new (std::nothrow) RtScene);
    if (!s) return set_err(RT_E_NOMEM, "out of memory");
    std::string err;
    const CompileOptions opt = compile_options_for_create(desc);
    int n = 0;
    if (opt.bvh_on_device) {  // the device builder needs its device before the scene is compiled
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_err(RT_E_DEVICE, "no HIP device available");
        if (device < 0 || device >= n) return set_err(RT_E_INVALID, "device index out of range");
        HIP_TRY(hipSetDevice(device));
    }
    int st = compile_scene(desc, &s->compiled, &err, opt);
    if (st != RT_OK) return set_err(st, err);
    s->content_digest = scene_digest(*desc);  // the description has been validated by the compiler
    s->held.assign(*desc);
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_err(RT_E_DEVICE, "no HIP device available");
    if (device < 0 || device >= n) return set_err(RT_E_INVALID, "device index out of range");
    s->device = device;
    HIP_TRY(hipSetDevice(device));
    if ((st = s->stream.create_non_blocking()) || (st = s->ev0.ensure()) || (st = s->ev1.ensure()) || (st = s->d_counters.reserve(sizeof(DeviceCounters))))
        return st;
    *out = s.release();
    return RT_OK;
}

void rt_scene_destroy(RtScene* s) { delete s; }  // ~RtScene sets the device

int rt_debug_live_resources(uint64_t out[4]) {
    if (!out) return rt::set_err(RT_E_INVALID, "rt_debug_live_resources: NULL argument");
    for (int k = 0; k < 4; k++) out[k] = rt::g_live[k].load();
    return RT_OK;
}

int rt_render_device(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                     double* d_rgba_out, void* stream) {
    int r = rt::render_replicas(scene, camera, params, 0, params ? params->thread_count : 0, d_rgba_out, stream);
    // whoever waits for this render's tail (rt_scene_set_tail_flag) is released at the latest here, errors included
    if (scene && scene->tail_flag) __atomic_store_n(scene->tail_flag, 1, __ATOMIC_RELEASE);
    return r;
}

int rt_scene_set_tail_flag(RtScene* scene, int32_t* flag) {
    if (!scene) return rt::set_err(RT_E_INVALID, "rt_scene_set_tail_flag: NULL scene");
    scene->tail_flag = flag;
    return RT_OK;
}

static int render_host_impl(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, double* rgba_out) {
    using namespace rt;
    if (!scene || !camera || !params || !rgba_out) return set_err(RT_E_INVALID, "rt_render: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    HIP_TRY(hipSetDevice(scene->device));
    uint32_t owned = owned_rows(camera->image_height, params);
    size_t bytes = size_t(owned) * camera->image_width * 4 * sizeof(double);
    if (bytes == 0) return RT_OK;
    return with_device_frame(bytes, rgba_out, bytes, [&](double* d_out) { return rt_render_device(scene, camera, params, d_out, nullptr); });
}

int rt_render(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, double* rgba_out) {
    int r = render_host_impl(scene, camera, params, rgba_out);
    if (scene && scene->tail_flag) __atomic_store_n(scene->tail_flag, 1, __ATOMIC_RELEASE);  // also on the early error returns
    return r;
}

int rt_debug_fuzzy_reflection(int device, uint32_t n, const double* reflected, const double* fuzz, const uint64_t* state, double* out, uint64_t* state_out) {
    using namespace rt;
    if (!n || !reflected || !fuzz || !state || !out || !state_out) return set_err(RT_E_INVALID, "rt_debug_fuzzy_reflection: NULL argument");
    HIP_TRY(hipSetDevice(device));
    DeviceBuffers buf;
    void *d_r = nullptr, *d_f = nullptr, *d_s = nullptr, *d_o = nullptr, *d_so = nullptr;
    int st;
    if ((st = buf.alloc(size_t(n) * 24, &d_r)) || (st = buf.alloc(size_t(n) * 8, &d_f)) || (st = buf.alloc(size_t(n) * 8, &d_s)) ||
        (st = buf.alloc(size_t(n) * 48, &d_o)) || (st = buf.alloc(size_t(n) * 16, &d_so))) return st;
    HIP_TRY(hipMemcpy(d_r, reflected, size_t(n) * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_f, fuzz, size_t(n) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s, state, size_t(n) * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_fuzzy_reflection, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, static_cast<const double*>(d_r), static_cast<const double*>(d_f),
                       static_cast<const unsigned long long*>(d_s), static_cast<double*>(d_o), static_cast<unsigned long long*>(d_so));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_o, size_t(n) * 48, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(state_out, d_so, size_t(n) * 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Diagnostic: traces ONE sample on the device and returns its radiance plus a per-bounce record
// (17 doubles, see k_trace_sample).  Returns the bounce count.
int rt_debug_trace_sample(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                          uint32_t tid, uint32_t x, uint32_t y, uint32_t sx, uint32_t sy,
                          double* rgb_out, double* trace_out, uint32_t max_bounces) {
    using namespace rt;
    if (!scene || !camera || !params || !rgb_out || !trace_out) return set_err(RT_E_INVALID, "NULL argument");
    RtScene* s = const_cast<RtScene*>(scene);
    HIP_TRY(hipSetDevice(s->device));
    DevBuf<double> d_buf;
    size_t n_d = 3 + size_t(max_bounces) * 17 + 1;
    if (int st = d_buf.reserve(n_d * sizeof(double))) return st;
    HIP_TRY(hipMemset(d_buf, 0, n_d * sizeof(double)));
    uint32_t* d_n = reinterpret_cast<uint32_t*>(d_buf + 3 + size_t(max_bounces) * 17);
    if (int st = with_tables(s, params->precision, [&](auto& ds) -> int {
            using R = typename std::decay_t<decltype(ds)>::Real;
            size_t lds = size_t(ds.view.stack_entries) * 64 * sizeof(int);
            hipLaunchKernelGGL((k_trace_sample<R>), dim3(1), dim3(64), lds, s->stream, ds.view, make_camera_view<R>(*camera, *params),
                               make_params_view<R>(*params, camera->image_height), tid, x, y, sx, sy, d_buf.get(), d_buf + 3, max_bounces, d_n);
            return RT_OK;
        }))
        return st;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<double> h(n_d);
    HIP_TRY(hipMemcpy(h.data(), d_buf, n_d * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(rgb_out, h.data(), 3 * sizeof(double));
    std::memcpy(trace_out, h.data() + 3, size_t(max_bounces) * 17 * sizeof(double));
    uint32_t n;
    std::memcpy(&n, h.data() + 3 + size_t(max_bounces) * 17, sizeof n);
    return int(n);
}

// Diagnostic: one path vertex per ray on the device (k_shade_rays).
int rt_debug_shade_rays(const RtScene* scene, const RtRenderParams* params, uint32_t variant, uint32_t n, const double* rays,
                        const uint64_t* states, double* out, uint64_t* state_out) {
    using namespace rt;
    if (!scene || !params || !rays || !states || !out || !state_out) return set_err(RT_E_INVALID, "rt_debug_shade_rays: NULL argument");
    if (variant > 2) return set_err(RT_E_INVALID, "rt_debug_shade_rays: variant is 0 (the render's), 1 (full) or 2 (simple)");
    if (n == 0) return RT_OK;
    RtScene* s = const_cast<RtScene*>(scene);
    const bool needs_full = s->compiled.needs_tex_interpreter || !s->compiled.volumes.empty();  // as render_typed picks
    if (variant == 2 && needs_full)
        return set_err(RT_E_INVALID, "rt_debug_shade_rays: the scene needs the full variant (texture interpreter or volumes)");
    const bool tex = variant == 1 || (variant == 0 && needs_full);
    HIP_TRY(hipSetDevice(s->device));
    DevBuf<double> d_rays, d_out;
    DevBuf<unsigned long long> d_states, d_state_out;
    const size_t out_bytes = size_t(n) * RT_SHADE_RAYS_STRIDE * sizeof(double);
    int st;
    if ((st = d_rays.reserve(size_t(n) * 6 * sizeof(double))) || (st = d_out.reserve(out_bytes)) ||
        (st = d_states.reserve(size_t(n) * 8)) || (st = d_state_out.reserve(size_t(n) * 8))) return st;
    HIP_TRY(hipMemcpy(d_rays, rays, size_t(n) * 6 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_states, states, size_t(n) * 8, hipMemcpyHostToDevice));
    if ((st = with_tables(s, params->precision, [&](auto& ds) -> int {
            using R = typename std::decay_t<decltype(ds)>::Real;
            const size_t lds = size_t(ds.view.stack_entries) * 256 * sizeof(int);  // as k_megakernel's
            if (lds > 160 * 1024) return set_err(RT_E_UNSUPPORTED, "mesh BVH too deep for the LDS traversal stack");
            const dim3 grid((n + 255u) / 256u), block(256);
            const ParamsView<R> pv = make_params_view<R>(*params, 0);
            if (tex) hipLaunchKernelGGL((k_shade_rays<R, true>), grid, block, lds, s->stream, ds.view, pv, n, d_rays.get(), d_states.get(), d_out.get(), d_state_out.get());
            else hipLaunchKernelGGL((k_shade_rays<R, false>), grid, block, lds, s->stream, ds.view, pv, n, d_rays.get(), d_states.get(), d_out.get(), d_state_out.get());
            return RT_OK;
        })))
        return st;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(state_out, d_state_out, size_t(n) * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_update(RtScene* s, const RtSceneDesc* desc, RtSceneUpdateInfo* info) {
    using namespace rt;
    const auto t_begin = std::chrono::steady_clock::now();
    if (info) *info = RtSceneUpdateInfo{};
    if (!s || !desc) return set_err(RT_E_INVALID, "rt_scene_update: NULL argument");
    // ---- host only (rt_desc.cpp): everything that can refuse the description, before any device state is touched ----
    UpdatePlan plan;
    int st = plan_scene_update(s->held, s->compiled, desc, &plan);
    if (st != RT_OK) return st;
    CompiledScene& cs = plan.cs;
    const std::vector<uint32_t>& moved = plan.moved;
    std::string err;
    // ---- device ----
    HIP_TRY(hipSetDevice(s->device));
    uint64_t bytes = 0;
    float kernel_ms = 0.f;
    std::unique_ptr<DeviceScene<double>> n64;
    std::unique_ptr<DeviceScene<float>> n32;
    const bool on_device = s->f64 || s->f32;
    if (on_device && !moved.empty()) {
        s->refit.resize(cs.mesh_geoms.size());
        for (uint32_t gi : moved) {
            const CompiledScene::MeshGeom& g = cs.mesh_geoms[gi];
            std::vector<int32_t> child2(2 * size_t(g.n_nodes)), child4(4 * size_t(g.n_nodes4));
            if (!s->refit[gi].tri_order) {  // relative references, once
                for (uint32_t i = 0; i < g.n_nodes; i++) { child2[2 * size_t(i)] = cs.nodes[g.node_base + i].c0; child2[2 * size_t(i) + 1] = cs.nodes[g.node_base + i].c1; }
                for (uint32_t i = 0; i < g.n_nodes4; i++)
                    for (int k = 0; k < 4; k++) child4[4 * size_t(i) + size_t(k)] = mesh_relative_child(cs.nodes4[g.node4_base + i].child[k], g);
            }
            if (!refit_mesh_upload(s->refit[gi], desc->meshes[g.mesh], cs.tri_order.data() + g.tri_base, child2.data(), g.n_nodes, child4.data(), g.n_nodes4,
                                   s->stream, &bytes, &err))
                return set_err(RT_E_DEVICE, err);
        }
    }
    if (on_device) {
        HIP_TRY(hipStreamSynchronize(s->stream));  // the vertex copies; DeviceScene::build uses the null stream and synchronises the device
        // The small tables first, uploaded afresh beside the old ones (a failure here leaves the scene as it was) ...
        if (s->f64) {
            n64 = std::make_unique<DeviceScene<double>>();
            if ((st = n64->build(cs, s->f64.get())) != RT_OK) return st;
            bytes += n64->buf.uploaded_bytes;
        }
        if (s->f32) {
            n32 = std::make_unique<DeviceScene<float>>();
            if ((st = n32->build(cs, s->f32.get())) != RT_OK) return st;
            bytes += n32->buf.uploaded_bytes;
        }
        // ... then the kernels.  From here on a device error leaves the mesh tables half written: the scene can only be destroyed.
        if (!moved.empty()) {
            HIP_TRY(hipEventRecord(s->ev0, s->stream));
            if (s->f64 && (st = refit_typed<double>(s, cs, moved, *s->f64)) != RT_OK) return st;
            if (s->f32 && (st = refit_typed<float>(s, cs, moved, *s->f32)) != RT_OK) return st;
            HIP_TRY(hipEventRecord(s->ev1, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            HIP_TRY(hipEventElapsedTime(&kernel_ms, s->ev0, s->ev1));
        }
    }
    // ---- commit ----
    if (n64) { n64->take_mesh_tables(*s->f64); s->f64 = std::move(n64); }
    if (n32) { n32->take_mesh_tables(*s->f32); s->f32 = std::move(n32); }
    s->compiled = std::move(cs);
    HeldDesc old = std::move(s->held);
    s->held.assign(*desc, &old, &plan.same);
    s->content_digest = scene_digest(*desc);
    s->generation++;
    if (info) {
        info->n_meshes_refit = uint32_t(moved.size());
        info->n_triangles_refit = plan.n_tris_moved;
        info->bytes_uploaded = bytes;
        info->refit_kernel_ms = double(kernel_ms);
        info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return RT_OK;
}

int rt_debug_scene_mesh(const RtScene* scene, uint32_t mesh, uint32_t f32, int32_t* children_out, uint32_t* cones_out, float* boxes_out,
                        uint32_t node_capacity, uint32_t* n_nodes_out, double* tris_out, uint32_t* tri_order_out, uint32_t tri_capacity,
                        uint32_t* n_tris_out) {
    using namespace rt;
    if (!scene || !n_nodes_out || !n_tris_out) return set_err(RT_E_INVALID, "rt_debug_scene_mesh: NULL argument");
    RtScene* s = const_cast<RtScene*>(scene);
    HIP_TRY(hipSetDevice(s->device));
    const CompiledScene::MeshGeom* g = nullptr;
    if (!mesh_export_range(s->compiled, mesh, &g)) return set_err(RT_E_INVALID, "rt_debug_scene_mesh: mesh index out of range");
    const MeshExportOut o{children_out, cones_out, boxes_out, node_capacity, n_nodes_out, tris_out, tri_order_out, tri_capacity, n_tris_out};
    return with_tables(s, f32 ? RT_PRECISION_F32 : RT_PRECISION_F64, [&](auto& ds) { return mesh_export_device(s->compiled, *g, ds, o); });
}

int rt_debug_scene_mesh_digest(const RtScene* scene, uint32_t f32, uint64_t out[8]) {
    using namespace rt;
    if (!scene || !out) return set_err(RT_E_INVALID, "rt_debug_scene_mesh_digest: NULL argument");
    RtScene* s = const_cast<RtScene*>(scene);
    HIP_TRY(hipSetDevice(s->device));
    const CompiledScene& cs = s->compiled;
    std::vector<char> h;
    auto digest_of = [&](const void* d_ptr, size_t bytes, uint64_t* o) -> int {
        h.resize(bytes);
        if (bytes) HIP_TRY(hipMemcpy(h.data(), d_ptr, bytes, hipMemcpyDeviceToHost));
        Digest g;
        g.bytes(h.data(), bytes);
        *o = g.value();
        return RT_OK;
    };
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (int st = with_tables(s, f32 ? RT_PRECISION_F32 : RT_PRECISION_F64, [&](auto& ds) -> int {
            using R = typename std::decay_t<decltype(ds)>::Real;
            const auto tables = digest_tables<R>(cs, ds.view.nodes, ds.view.nodes4, ds.view.nodes4q, ds.view.tris, ds.view.attrs, ds.view.mesh_bounds,
                                                 ds.view.mesh_op_recs);
            for (int k = 0; k < 7; k++)
                if (int st = digest_of(tables[k].first, tables[k].second, &out[k])) return st;
            return RT_OK;
        }))
        return st;
    out[7] = s->generation;
    return RT_OK;
}

// ---- First-hit AOVs (kernel, denoiser and its entry points: rt_aov.hip) ------------------------------------------------
int rt_render_aov_device(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                         double* d_aov_out, void* stream) {
    return rt::render_aov_replicas(scene, camera, params, n_replicas, d_aov_out, stream);
}

int rt_render_aov(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                  double* aov_out) {
    using namespace rt;
    if (!scene || !camera || !params || !aov_out) return set_err(RT_E_INVALID, "rt_render_aov: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    HIP_TRY(hipSetDevice(scene->device));
    const size_t bytes = size_t(owned_rows(camera->image_height, params)) * camera->image_width * kAovChannels * sizeof(double);
    if (bytes == 0) return rt::render_aov_replicas(scene, camera, params, n_replicas, aov_out, nullptr);  // argument checks only
    return with_device_frame(bytes, aov_out, bytes, [&](double* d_out) { return rt::render_aov_replicas(scene, camera, params, n_replicas, d_out, nullptr); });
}

// ---------------------------------------------------------------------------------------------
// Light groups (include/rt_mi355.h)
// ---------------------------------------------------------------------------------------------
static int light_groups_impl(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, const RtLightGroups* groups,
                             double* d_groups_out, double* d_rgba_out, void* stream) {
    using namespace rt;
    if (!scene || !camera || !params || !groups || !d_groups_out) return set_err(RT_E_INVALID, "rt_render_light_groups: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    RtScene* s = const_cast<RtScene*>(scene);
    const uint32_t G = groups->n_groups, M = uint32_t(s->compiled.materials.size());
    if (G < 1 || G > RT_LIGHT_GROUPS_MAX) return set_err(RT_E_INVALID, "RtLightGroups: n_groups outside 1 .. RT_LIGHT_GROUPS_MAX");
    if (groups->n_materials != M) return set_err(RT_E_INVALID, "RtLightGroups: n_materials differs from the scene's (" + std::to_string(M) + ")");
    if (M && !groups->material_group) return set_err(RT_E_INVALID, "RtLightGroups: material_group is NULL");
    if (groups->background_group >= G) return set_err(RT_E_INVALID, "RtLightGroups: background_group >= n_groups");
    if (groups->unlit_group >= G) return set_err(RT_E_INVALID, "RtLightGroups: unlit_group >= n_groups");
    for (uint32_t m = 0; m < M; m++)
        if (groups->material_group[m] >= G) return set_err(RT_E_INVALID, "RtLightGroups: material_group[" + std::to_string(m) + "] >= n_groups");
    if (params->pipeline == RT_PIPELINE_MEGAKERNEL) return set_err(RT_E_UNSUPPORTED, "light groups run the wavefront scheduler: RT_PIPELINE_MEGAKERNEL is not supported");
    if (params->max_depth == 0) return set_err(RT_E_UNSUPPORTED, "light groups with max_depth = 0");
    if (params->collect_stats) return set_err(RT_E_UNSUPPORTED, "light groups have no counting kernels (collect_stats)");
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t owned = owned_rows(camera->image_height, params);
    if (owned == 0) return RT_OK;
    // group of a path that ends on material m, of a miss, of an exhausted depth (rt_wavefront.h WfGroupLG)
    std::vector<uint8_t> table(size_t(M) + 2);
    for (uint32_t m = 0; m < M; m++) {
        const int32_t t = s->compiled.materials[m].type;
        table[m] = (t == RT_MAT_EMISSIVE || t == RT_MAT_NORMAL_DEBUG) ? groups->material_group[m] : uint8_t(groups->unlit_group);
    }
    table[M] = uint8_t(params->has_background ? groups->background_group : groups->unlit_group);
    table[M + 1] = uint8_t(groups->unlit_group);
    LightGroupPass lg;
    lg.n_groups = G;
    lg.n_materials = M;
    lg.table = table.data();
    lg.d_groups_out = d_groups_out;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
    const uint32_t T = params->thread_count;
    return with_tables(s, params->precision, [&](auto& ds) { return render_wavefront(s, ds, *camera, *params, owned, 0, T, d_rgba_out, st, lg); });
}

int rt_render_light_groups_device(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, const RtLightGroups* groups,
                                  double* d_groups_out, double* d_rgba_out_or_null, void* stream) {
    int r = light_groups_impl(scene, camera, params, groups, d_groups_out, d_rgba_out_or_null, stream);
    if (scene && scene->tail_flag) __atomic_store_n(scene->tail_flag, 1, __ATOMIC_RELEASE);  // as rt_render_device
    return r;
}

int rt_render_light_groups(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, const RtLightGroups* groups,
                           double* groups_out, double* rgba_out_or_null) {
    using namespace rt;
    if (!scene || !camera || !params || !groups || !groups_out) return set_err(RT_E_INVALID, "rt_render_light_groups: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    if (groups->n_groups < 1 || groups->n_groups > RT_LIGHT_GROUPS_MAX) return set_err(RT_E_INVALID, "RtLightGroups: n_groups outside 1 .. RT_LIGHT_GROUPS_MAX");
    HIP_TRY(hipSetDevice(scene->device));
    const size_t frame = size_t(owned_rows(camera->image_height, params)) * camera->image_width * 4 * sizeof(double);
    if (frame == 0) return RT_OK;
    // the group frames, then the ordinary frame
    return with_device_frame(frame * (size_t(groups->n_groups) + 1), groups_out, frame * groups->n_groups, [&](double* d_buf) -> int {
        double* d_frame = d_buf + (frame / sizeof(double)) * groups->n_groups;
        if (int st = rt_render_light_groups_device(scene, camera, params, groups, d_buf, rgba_out_or_null ? d_frame : nullptr, nullptr)) return st;
        if (!rgba_out_or_null) return RT_OK;
        const hipError_t e = hipMemcpy(rgba_out_or_null, d_frame, frame, hipMemcpyDeviceToHost);
        return e == hipSuccess ? int(RT_OK) : set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    });
}

int rt_light_mix_device(int device, const double* d_groups, uint32_t n_groups, uint32_t w, uint32_t h, const double* tints,
                        double* d_rgba_out, void* stream) {
    using namespace rt;
    if (!d_groups || !tints || !d_rgba_out) return set_err(RT_E_INVALID, "rt_light_mix: NULL argument");
    if (n_groups < 1 || n_groups > RT_LIGHT_GROUPS_MAX) return set_err(RT_E_INVALID, "rt_light_mix: n_groups outside 1 .. RT_LIGHT_GROUPS_MAX");
    const uint64_t npix = uint64_t(w) * h;
    if (npix == 0) return RT_OK;
    HIP_TRY(hipSetDevice(device));
    LightMixTints t{};
    for (uint32_t k = 0; k < 3 * n_groups; k++) t.v[k] = tints[k];
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_light_mix, dim3(uint32_t((npix + 255) / 256)), dim3(256), 0, st, d_groups, n_groups, npix, t, d_rgba_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_light_mix(int device, const double* groups, uint32_t n_groups, uint32_t w, uint32_t h, const double* tints, double* rgba_out) {
    using namespace rt;
    if (!groups || !tints || !rgba_out) return set_err(RT_E_INVALID, "rt_light_mix: NULL argument");
    if (n_groups < 1 || n_groups > RT_LIGHT_GROUPS_MAX) return set_err(RT_E_INVALID, "rt_light_mix: n_groups outside 1 .. RT_LIGHT_GROUPS_MAX");
    const size_t frame = size_t(w) * h * 4 * sizeof(double);
    if (frame == 0) return RT_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> d_buf;  // the group frames, then the mix
    if (int st = d_buf.reserve(frame * (size_t(n_groups) + 1))) return st;
    double* d_out = d_buf + (frame / sizeof(double)) * n_groups;
    hipError_t e = hipMemcpy(d_buf, groups, frame * n_groups, hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    if (int st = rt_light_mix_device(device, d_buf, n_groups, w, h, tints, d_out, nullptr)) return st;
    e = hipMemcpy(rgba_out, d_out, frame, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    return RT_OK;
}

// ---- Renders along ray tables, irradiance and probe bakes: rt::table_call with the call's description and the mode's pass ----
int rt_render_rays(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, const RtRenderParams* params, double* rgba_out) {
    return rt::table_call(scene, n, params, rgba_out, true, nullptr,
                          {"rt_render_rays", {origins, "origins", 24}, {dirs, "dirs", 24}, "rgba_out", 32, "ray table", "ray"}, rt::ray_table_pass);
}
int rt_render_rays_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs, const RtRenderParams* params,
                          double* d_rgba_out, void* stream) {
    return rt::table_call(scene, n, params, d_rgba_out, false, stream,
                          {"rt_render_rays_device", {d_origins, "origins", 24}, {d_dirs, "dirs", 24}, "rgba_out", 32, "ray table", "ray"}, rt::ray_table_pass);
}

int rt_bake_irradiance(const RtScene* scene, uint64_t n, const double* positions, const double* normals, const RtRenderParams* params, double* rgba_out) {
    return rt::table_call(scene, n, params, rgba_out, true, nullptr,
                          {"rt_bake_irradiance", {positions, "positions", 24}, {normals, "normals", 24}, "rgba_out", 32, "point table", "point"},
                          rt::point_table_pass<false>);
}
int rt_bake_irradiance_device(const RtScene* scene, uint64_t n, const double* d_positions, const double* d_normals, const RtRenderParams* params,
                              double* d_rgba_out, void* stream) {
    return rt::table_call(scene, n, params, d_rgba_out, false, stream,
                          {"rt_bake_irradiance_device", {d_positions, "positions", 24}, {d_normals, "normals", 24}, "rgba_out", 32, "point table", "point"},
                          rt::point_table_pass<false>);
}
int rt_bake_irradiance_hits_device(const RtScene* scene, uint64_t n, const RtRayHit* d_hits, const RtRenderParams* params, double* d_rgba_out,
                                   void* stream) {
    return rt::table_call(scene, n, params, d_rgba_out, false, stream,
                          {"rt_bake_irradiance_hits_device", {d_hits, "hits", sizeof(RtRayHit)}, {}, "rgba_out", 32, "point table", "point"},
                          rt::point_table_pass<true>, [=](uint64_t off, uint32_t m, double* d_out, hipStream_t st) { return rt::points_mask(d_hits + off, m, d_out, st); });
}

int rt_bake_probes(const RtScene* scene, uint64_t n, const double* positions, const RtRenderParams* params, double* sh_out) {
    return rt::table_call(scene, n, params, sh_out, true, nullptr,
                          {"rt_bake_probes", {positions, "positions", 24}, {}, "sh_out", 288, "probe table", "probe"}, rt::probe_table_pass);
}
int rt_bake_probes_device(const RtScene* scene, uint64_t n, const double* d_positions, const RtRenderParams* params, double* d_sh_out, void* stream) {
    return rt::table_call(scene, n, params, d_sh_out, false, stream,
                          {"rt_bake_probes_device", {d_positions, "positions", 24}, {}, "sh_out", 288, "probe table", "probe"}, rt::probe_table_pass);
}

int rt_sh_irradiance_device(int device, const double* d_sh, uint64_t n_probes, const uint32_t* d_probe, const double* d_normals, uint64_t m,
                            double* d_rgba_out, void* stream) {
    using namespace rt;
    if (m == 0) return RT_OK;
    if (!d_probe || !d_normals || !d_rgba_out || (n_probes && !d_sh)) return set_err(RT_E_INVALID, "rt_sh_irradiance_device: NULL argument");
    if (m >= (1ull << 31) || n_probes >= (1ull << 31)) return set_err(RT_E_INVALID, "rt_sh_irradiance_device: m and n_probes must be below 2^31");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_sh_irradiance, dim3(uint32_t((m + 255) / 256)), dim3(256), 0, st, d_sh, n_probes, d_probe, d_normals, m, d_rgba_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_sh_irradiance(int device, const double* sh, uint64_t n_probes, const uint32_t* probe, const double* normals, uint64_t m, double* rgba_out) {
    using namespace rt;
    if (m == 0) return RT_OK;
    if (!probe || !normals || !rgba_out || (n_probes && !sh)) return set_err(RT_E_INVALID, "rt_sh_irradiance: NULL argument");
    if (m >= (1ull << 31) || n_probes >= (1ull << 31)) return set_err(RT_E_INVALID, "rt_sh_irradiance: m and n_probes must be below 2^31");
    for (uint64_t j = 0; j < m; j++)
        if (probe[j] >= n_probes) return set_err(RT_E_INVALID, "rt_sh_irradiance: probe[" + std::to_string(j) + "] = " + std::to_string(probe[j]) + " is not below n_probes");
    HIP_TRY(hipSetDevice(device));
    const size_t b_sh = size_t(n_probes) * 36 * sizeof(double), b_n = size_t(m) * 24, b_out = size_t(m) * 32, b_p = size_t(m) * 4;
    DevBuf<double> d_buf;  // coefficients, normals, answers, then the indices
    if (int st = d_buf.reserve(b_sh + b_n + b_out + b_p)) return st;
    double* d_sh = d_buf;
    double* d_n = d_sh + b_sh / sizeof(double);
    double* d_out = d_n + b_n / sizeof(double);
    uint32_t* d_p = reinterpret_cast<uint32_t*>(d_out + b_out / sizeof(double));
    auto copy = [](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) -> int {
        const hipError_t e = hipMemcpy(dst, src, bytes, kind);
        return e == hipSuccess ? int(RT_OK) : set_err(RT_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    };
    if (int st = copy(d_sh, sh, b_sh, hipMemcpyHostToDevice)) return st;
    if (int st = copy(d_n, normals, b_n, hipMemcpyHostToDevice)) return st;
    if (int st = copy(d_p, probe, b_p, hipMemcpyHostToDevice)) return st;
    if (int st = rt_sh_irradiance_device(device, d_sh, n_probes, d_p, d_n, m, d_out, nullptr)) return st;
    return copy(rgba_out, d_out, b_out, hipMemcpyDeviceToHost);
}

int rt_get_stats(const RtScene* scene, RtRenderStats* out) {
    if (!scene || !out) return rt::set_err(RT_E_INVALID, "rt_get_stats: NULL argument");
    *out = scene->stats;
    return RT_OK;
}

}  // extern "C"

// query_search_pass as rt_query.hip calls it (rt_scene_host.h): plain functions, and last in the file.  The compiler emits a
// kernel where it is first named; named from here, make_search_setup<R> is first named inside render_wavefront's instantiation,
// as it always was, and the search kernels keep their places in the code object.  An explicit instantiation of the template
// would name them where it stands, float and double side by side.
namespace rt {
int query_search_pass(RtScene* s, DeviceScene<float>& ds, const PathPool<float>& pl, uint32_t m, hipStream_t stream) {
    return query_search_pass<float>(s, ds, pl, m, stream);
}
int query_search_pass(RtScene* s, DeviceScene<double>& ds, const PathPool<double>& pl, uint32_t m, hipStream_t stream) {
    return query_search_pass<double>(s, ds, pl, m, stream);
}
}  // namespace rt
