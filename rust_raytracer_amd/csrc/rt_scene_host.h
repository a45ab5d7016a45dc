// rt_scene_host.h — host only: RtScene as the translation units of the library see it (rt_kernels.hip, rt_query.hip,
// rt_point.hip, rt_bake.hip, rt_lightmap.hip): the scene's tables on the device, its workspaces, and the helpers the host
// sides of the subsystems share (the chunk loop, the lazily built tables, the argument checks of a query).  It does not
// include rt_wavefront.h: the pools and counters it names are the plain structs of rt_pool.h.  What names a wavefront kernel
// or builds the pool stays defined in rt_kernels.hip and is only declared here.  A client of the
// renderer (rt_accum.hip) does not include this header: it goes through rt_render.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <variant>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_compile.h"
#include "rt_desc.h"
#include "rt_device.h"
#include "rt_owned.h"
#include "rt_pool.h"
#include "rt_refit.h"
#include "rt_tables.h"

namespace rt {

// Device copies of host tables; every table is a buffer of its own, so that rt_scene_update can move the mesh tables over.
struct DeviceBuffers {
    std::vector<DevBuf<char>> allocs;
    uint64_t uploaded_bytes = 0;
    // takes over an allocation of `from` (rt_scene_update: the mesh tables stay where they are)
    void adopt(DeviceBuffers& from, const void* p) {
        auto it = std::find_if(from.allocs.begin(), from.allocs.end(), [p](const DevBuf<char>& b) { return b.get() == p; });
        if (it == from.allocs.end()) return;
        allocs.push_back(std::move(*it));
        from.allocs.erase(it);
    }
    // `bytes` of device memory that live as long as this object
    template <typename T> int alloc(size_t bytes, T** out) {
        allocs.emplace_back();
        if (int st = allocs.back().reserve(bytes)) return st;
        *out = reinterpret_cast<T*>(allocs.back().get());
        return RT_OK;
    }
    template <typename T> int upload(const std::vector<T>& v, const T** out) {
        *out = nullptr;
        T* p = nullptr;
        if (int st = alloc((v.empty() ? 1 : v.size()) * sizeof(T), &p)) return st;
        if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        uploaded_bytes += v.size() * sizeof(T);
        *out = p;
        return RT_OK;
    }
};

// Scene tables in arithmetic type R on the device.  build and take_mesh_tables are defined in rt_kernels.hip and
// instantiated there for float and double: one translation unit compiles the uploads.
template <typename R>
struct DeviceScene {
    using Real = R;
    DeviceBuffers buf;
    SceneView<R> view{};

    // The tables are derived on the host (rt_tables.cpp); this uploads them, one buffer each.
    // keep != NULL (rt_scene_update): the mesh tables (BVH nodes of every format, triangle records, attributes) are not
    // derived and uploaded but stay the arrays of `keep`, which the refit kernels rewrite; take_mesh_tables() moves their
    // ownership over once the update is certain.
    int build(const CompiledScene& cs, const DeviceScene<R>* keep = nullptr);
    void take_mesh_tables(DeviceScene<R>& from);
};

// The arrays of a WfPool<R> and the queues over its slots (build_pool).  A render works on a pair of them (the second one,
// 3/4 of the slots, is the destination of the first tail compaction, after which the two take turns), a ray query on the
// first of a pair; the arithmetic type a workspace's pools were built for is the alternative its variant holds.
template <typename R>
struct PathPool {
    WfPool<R> view{};                             // array bases and capacity, as the kernels take them
    WfPool<R>* dev = nullptr;                     // the same descriptor in device memory (k_wf_shade re-reads the array bases from it)
    uint32_t* queue[2] = {nullptr, nullptr};
    uint32_t* mesh_queue = nullptr;
    std::vector<DevBuf<char>> owned;              // what all of the above point at
};
template <typename R> using PoolPair = std::array<PathPool<R>, 2>;
using AnyPools = std::variant<std::monostate, PoolPair<float>, PoolPair<double>>;

// What run_chunks keeps between calls: the host variants' staging buffer (inputs and results of one chunk; grows only) and
// the pair of events that times a chunk.
struct ChunkStage {
    DevBuf<char> staging;
    Event ev0, ev1;
};

}  // namespace rt

struct RtScene {
    int device = -1;  // set once rt_scene_create has chosen it; nothing is allocated before
    rt::CompiledScene compiled;
    // Both precisions are materialised lazily on first use (with_tables).
    std::unique_ptr<rt::DeviceScene<double>> f64;
    std::unique_ptr<rt::DeviceScene<float>> f32;
    rt::Stream stream;
    rt::Event ev0, ev1;
    rt::DevBuf<rt::DeviceCounters> d_counters;
    RtRenderStats stats{};
    int32_t* tail_flag = nullptr;  // rt_scene_set_tail_flag: set to 1 when a render stops filling the GPU (frame pipelining)
    uint64_t content_digest = 0;   // of everything the description points at (rt::scene_digest): checkpoints name their scene by it
    // rt_scene_update: the description the scene holds, a counter of its updates (accumulators belong to one generation) and
    // the device-side refit state per distinct mesh (CompiledScene::mesh_geoms order; empty until a mesh is first moved)
    rt::HeldDesc held;
    uint64_t generation = 0;
    std::vector<rt::RefitMesh> refit;
    // wavefront pipeline resources (allocated on first use, reused between renders)
    struct Wavefront {
        rt::AnyPools pools;
        rt::DevBuf<uint2> mesh_spill;      // k_wf_mesh: stack levels beyond the LDS part
        rt::DevBuf<rt::WfCounters> d_ctr;
        rt::PinnedBuf<rt::WfCounters> h_ctr;
        rt::DevBuf<double> sample_L, acc;
        // light-group renders (rt_render_light_groups): group byte per sample, running sums per (group, pixel), terminal table
        rt::DevBuf<uint8_t> sample_G, lg_table;
        rt::DevBuf<double> acc_g;
        rt::Event ev_res[2];
        std::vector<rt::Event> events;
    } wf;
    // ray queries (rt_trace_rays / rt_occluded): a workspace of their own, allocated by the first query, so that a query
    // between two progressive passes never makes wf_ensure re-allocate the render's pool
    struct Query {
        rt::AnyPools pools;                // [0]: ray and hit-record arrays only (the search kernels read nothing else); grows only
        rt::DevBuf<uint2> mesh_spill;
        rt::DevBuf<rt::WfCounters> d_ctr;
        rt::PinnedBuf<rt::WfCounters> h_ctr;
        rt::DevBuf<int32_t> op_node;       // CompiledScene::op_node / ::tri_order of generation `tables_generation`
        rt::DevBuf<uint32_t> tri_order;
        uint64_t tables_generation = ~0ull;
        rt::ChunkStage stage;
        RtRayQueryStats stats{};
    } rq;
    // ambient-occlusion bakes (rt_bake_visibility): stats of their own (rt_ray_query_stats is not theirs to change)
    struct Bake {
        rt::ChunkStage stage;
        RtRayQueryStats stats{};
    } bake;
    // renders along ray tables, irradiance and probe bakes (rt_render_rays, rt_bake_irradiance, rt_bake_probes): the host variants' staging buffer; the kernels run on the render's workspace (wf)
    struct Rays {
        rt::ChunkStage stage;
    } rays;
    // point queries (rt_closest_points): the per-chain scale table in the arithmetic type of `scale_precision`, as of generation
    // `scale_generation`, and stats of their own; op_node / tri_order are the ray queries' tables (rq)
    struct Points {
        rt::DevBuf<char> chain_scale;
        uint64_t scale_generation = ~0ull;
        uint32_t scale_precision = 0;
        rt::ChunkStage stage;
        RtRayQueryStats stats{};
    } points;
    // lightmaps (rt_lightmap_texels, rt_bake_lightmap; rt_lightmap.hip): the bins of the rasteriser, the records and
    // images of the stages between rasterisation and the caller's buffers, three events; op_node / tri_order are rq's
    struct Lightmap {
        rt::DevBuf<uint32_t> tile_count, tile_offset, tile_cursor, refs, counts;
        rt::DevBuf<unsigned long long> totals;
        rt::DevBuf<char> scan_temp;
        rt::DevBuf<RtRayHit> hits;
        rt::DevBuf<RtBakeResult> vis;
        rt::DevBuf<double> rgba_a, rgba_b, rgba_o;
        rt::DevBuf<uint8_t> cov_a, cov_b, cov_c;
        rt::Event ev[3];
        RtLightmapStats stats{};
    } lm;
    ~RtScene() { if (device >= 0) (void)hipSetDevice(device); }  // before the members go: the owners do not switch devices
};

namespace rt {

inline uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return uint32_t(std::strtoul(v, nullptr, 10));
}

// Makes sure the scene's tables in the arithmetic of `precision` are on the device (built on first use), then f(tables).
template <typename F>
int with_tables(RtScene* s, uint32_t precision, F&& f) {
    auto go = [&](auto& slot) -> int {
        if (!slot) {
            auto ds = std::make_unique<typename std::decay_t<decltype(slot)>::element_type>();
            if (int r = ds->build(s->compiled)) return r;
            slot = std::move(ds);
        }
        return f(*slot);
    };
    return precision == RT_PRECISION_F32 ? go(s->f32) : go(s->f64);
}

// n items in chunks of at most `chunk`: launch(off, m, d_in, d_out) enqueues the kernels of the m items from `off` on.
// `in` / out: the arrays and their bytes per item; an input array may be NULL.  host: they are host arrays and go through
// the staging buffer, which is sized by the largest chunk and laid out inputs first, then the output (a NULL input keeps its
// place); otherwise the kernels work on them where they are.  One synchronise per chunk; the events span the launches, not
// the copies.
struct ChunkArray { const void* p; size_t each; };
struct ChunkTimes { double ms = 0.0; uint32_t n_chunks = 0; };
template <typename F>
int run_chunks(ChunkStage& cs, uint64_t n, uint32_t chunk, bool host, const std::vector<ChunkArray>& in, void* out, size_t out_each,
               hipStream_t stream, F&& launch, ChunkTimes* times) {
    const size_t cap = size_t(std::min<uint64_t>(n, chunk));
    size_t each_all = out_each;
    for (const ChunkArray& a : in) each_all += a.each;
    if (host)
        if (int st = cs.staging.reserve(cap * each_all)) return st;
    if (int st = cs.ev0.ensure()) return st;
    if (int st = cs.ev1.ensure()) return st;
    std::vector<const void*> d_in(in.size());
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint32_t m = uint32_t(std::min<uint64_t>(chunk, n - off));
        char* const h_out = static_cast<char*>(out) + off * out_each;
        size_t at = 0;  // in the staging buffer
        for (size_t i = 0; i < in.size(); i++) {
            const char* src = in[i].p ? static_cast<const char*>(in[i].p) + off * in[i].each : nullptr;
            if (host && src) {
                HIP_TRY(hipMemcpyAsync(cs.staging + at, src, size_t(m) * in[i].each, hipMemcpyHostToDevice, stream));
                src = cs.staging + at;
            }
            d_in[i] = src;
            at += cap * in[i].each;
        }
        char* const d_out = host ? cs.staging + at : h_out;
        HIP_TRY(hipEventRecord(cs.ev0, stream));
        if (int st = launch(off, m, d_in.data(), static_cast<void*>(d_out))) return st;
        HIP_TRY(hipEventRecord(cs.ev1, stream));
        if (host) HIP_TRY(hipMemcpyAsync(h_out, d_out, size_t(m) * out_each, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, cs.ev0, cs.ev1));
        times->ms += ms;
        times->n_chunks++;
    }
    return RT_OK;
}

template <typename R>
static void record_query_stats(RtRayQueryStats& stats, const ChunkTimes& t, uint64_t rays) {
    stats = RtRayQueryStats{};
    stats.kernel_ms = t.ms;
    stats.rays = rays;
    stats.n_chunks = t.n_chunks;
    stats.precision = sizeof(R) == 8 ? RT_PRECISION_F64 : RT_PRECISION_F32;
}

// Argument checks shared by the entry points, then run(scene, tables of `precision` on the device).
template <typename F>
static int ray_query_run(const RtScene* scene, uint32_t precision, const char* who, F&& run) {
    if (!scene) return set_err(RT_E_INVALID, std::string(who) + ": NULL scene");
    if (precision != RT_PRECISION_F64 && precision != RT_PRECISION_F32) return set_err(RT_E_INVALID, std::string(who) + ": precision must be RT_PRECISION_F64 or RT_PRECISION_F32");
    if (!scene->compiled.volumes.empty())
        return set_err(RT_E_UNSUPPORTED, std::string(who) + ": ray queries do not support scenes with volumes (a medium gives no deterministic surface)");
    RtScene* s = const_cast<RtScene*>(scene);  // workspace + lazily built tables; the scene data itself is immutable
    HIP_TRY(hipSetDevice(s->device));
    return with_tables(s, precision, [&](auto& ds) -> int { return run(s, ds); });
}

// RtRayHit records as strided points: where the first record's position, normal and flags are, and the bytes from one record to
// the next.
struct HitPoints {
    const unsigned char *pos, *nrm, *flags;
    uint32_t stride;
};
inline HitPoints hit_points(const RtRayHit* hits) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(hits);
    return {base + offsetof(RtRayHit, pos), base + offsetof(RtRayHit, normal), base + offsetof(RtRayHit, flags), uint32_t(sizeof(RtRayHit))};
}

// ---- Defined in rt_kernels.hip ----
// Builds `pl` for `capacity` slots: rays and hit records, `full`: + the rest of the path state and the descriptor's device
// copy; n_queues queues and (with any queue) the mesh queue.  Instantiated there for float and double.
template <typename R>
int build_pool(PathPool<R>& pl, uint32_t capacity, bool full, int n_queues, const char* nomem);
// One pass of the scene's search kernels over slots 0 .. m-1 of the query pool.  Two plain functions over the template
// query_search_pass<R> of rt_kernels.hip, not its explicit instantiations: see the end of that file.
int query_search_pass(RtScene* s, DeviceScene<float>& ds, const PathPool<float>& pl, uint32_t m, hipStream_t stream);
int query_search_pass(RtScene* s, DeviceScene<double>& ds, const PathPool<double>& pl, uint32_t m, hipStream_t stream);

// One call of a table mode's entry point `who`.  a / b: the input arrays as the caller passed them (name NULL: the entry point
// has no such array; each: bytes per entry), out_name / out_each: the same of the output; what / unit: "ray table" / "ray".
struct TableArray {
    const void* p;
    const char* name;
    size_t each;
};
struct TableCall {
    const char* who;
    TableArray a, b;
    const char* out_name;
    size_t out_each;
    const char *what, *unit;
};
// The rules the table modes share, checked before the device is touched (rt_kernels.hip).
int table_render_check(const RtScene* scene, uint64_t n, const RtRenderParams* params, const void* out, const TableCall& c);

// ---- Defined in rt_query.hip ----
// op -> node and leaf slot -> triangle tables of the scene as it stands (uploaded again after an rt_scene_update), in s->rq:
// ray queries, point queries and lightmaps read them.
int rq_tables(RtScene* s, hipStream_t stream);
// Items per chunk of a ray or point query (RT_RQ_CHUNK).
uint32_t rq_chunk();

}  // namespace rt
