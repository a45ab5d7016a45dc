// rtrace — command-line driver with the reference's interface (src/main.rs:25-88): same flags
// (README.md:21-43), same scene DSL, same console lines, writes `out.png` (ACES + sRGB, 8-bit).
// The one thing that changed is line 75 of the reference's main.rs: instead of
// `camera.render(world, lights, &mut buf)` the frame comes from librt_mi355.so (rt_render).
//
// New, optional flags (ignored by the reference's parser, so command lines stay compatible):
//   --seed=<u64>  --gpus=<n>  --precision=f64|f32  --pipeline=auto|mega|wavefront  --bvh=host|device
//   --progressive=<n>  --checkpoint=<file>  --time-limit=<seconds>  --denoise=<iterations>
//   --noise-threshold=<x>  --adaptive-min=<k>  --adaptive-check=<m>  --adaptive-radius=<r>
//   --light-groups[=<max>]  --light-mix=<w0>,<w1>,...  --sequence=<scene1>[,<scene2>...]  --pick=<x>,<y>[:<x>,<y>...]
//   --ao=<samples>[:<max_distance>]  --probe=<x>,<y>,<z>[:<width>]  --irradiance  --sh-probe=<x>,<y>,<z>[:<x>,<y>,<z>...]
//   --nearest=<x>,<y>,<z>[:<x>,<y>,<z>...]  --lightmap=<k>:<width>[x<height>][:<passes>]
// --lightmap=<k>:<width>[x<height>][:<passes>] renders no frame: the irradiance lightmap of the k-th mesh op of the program over
// the mesh's own UVs (rt_bake_lightmap: rasterised, baked and dilated on the device) with the run's -s, -t, depth, bias, seed
// and precision, written to out_lightmap.png through the output stage of out.png; row 0 of the file is v near 0.
// --sh-probe=<x>,<y>,<z>[:...] renders nothing: an SH radiance probe is baked at each named position (rt_bake_probes) with the
// run's -s, -t, depth, bias, seed and precision and its nine RGB coefficients are printed, one line per coefficient.
// --irradiance also writes out_irradiance.png: the --pick ray of every pixel is cast on the device (rt_trace_rays_device) and the
// cosine-weighted mean of the radiance arriving at every first hit is baked with the run's -s, -t, depth, bias, seed and
// precision (rt_bake_irradiance_hits_device; the hit records never leave the device) and written through the output stage of
// out.png; a pixel that sees no surface is black.  A scene with volumes is refused before anything is rendered.  One more console
// line; out.png and the other console lines are those of a run without the flag.
// --probe=<x>,<y>,<z>[:<width>] renders no frame: an equirectangular light probe at that point (+y up, the centre column looking
// along -z; width 512 by default, height = width / 2) is rendered with rt_render_rays along the rays of rth_probe_rays, with the
// run's -s, -t, depth, bias, seed and precision, and written to out_probe.png through the output stage of out.png.  There is no
// pixel filter: every sample of a texel goes along the texel's centre ray.
// --pick=<x>,<y>[:...] renders nothing: the ray through the centre of each named pixel (no lens, no jitter) is cast with
// rt_trace_rays and one line per pixel is printed: node, node type, material, triangle, t, position.
// --ao=<samples>[:<max_distance>] also writes out_ao.png: the --pick ray of every pixel is cast on the device
// (rt_trace_rays_device), the visibility of every first hit is baked with the run's seed (rt_bake_visibility_hits_device; the
// hit records never leave the device) and written as grey through the sRGB curve, without ACES; a pixel that sees no surface is
// white.  A scene with volumes is refused before anything is rendered.  One more console line; out.png and the other console lines are those of a run without the flag.
// With --progressive=n the frame is rendered in passes of n replicas (rt_accum_*, one GPU); after each pass out.png shows
// the estimate so far (tone-mapped on the device), the final out.png is the one a run without the flag writes.
// --checkpoint saves the accumulator after every pass (<file>.tmp, then renamed) and resumes from <file> at start-up;
// --time-limit stops after the first pass that ends past the limit (measured from the start of the process).
// --denoise=n also writes out_denoised.png: the frame (with --progressive: the estimate after every pass, and the final
// frame) through the a-trous filter of rt_denoise with n iterations, guided by first-hit AOVs of one replica.  out.png
// and the console lines are those of a run without the flag.
// --noise-threshold=x turns adaptive sampling on (rt_accum_set_adaptive): the frame is rendered in passes (of --progressive
// replicas, else of the check interval) until every pixel has converged or all replicas are done; out.png is the final
// estimate, out_samples.png shows each pixel's share n / T of the replicas in grey, and one more console line gives the
// samples rendered and the pixels stopped.  Works with --checkpoint, --time-limit and --denoise.
// --light-groups[=max] also writes out_light_<g>.png, one frame per light group of the automatic assignment
// (rt_light_groups_auto: group 0 = everything that does not emit, then one group per Emissive material, then the background),
// all from the one render that gives out.png (rt_render_light_groups), and prints one line per group.  --light-mix=w0,w1,...
// also writes out_mixed.png = sum_g w_g * group g (rt_light_mix; groups without a weight count once).  out.png and the other
// console lines are those of a run without the flags.
// --sequence=<scene1>[,<scene2>...] renders <scene> to out.png as without the flag, then gives the SAME device scene the numbers of
// each following scene file (rt_scene_update: same structure, other transforms / colours / lights / vertex positions; mesh BVHs
// are refitted on the device, not rebuilt) and writes out_0001.png, out_0002.png, ... with one console line per frame (meshes
// refit, triangles, update time).  A file of another structure stops the run with the library's message.  One GPU, whole frames.
// With --gpus=n the frame is row-tiled in interleaved bands (rth_band_rows: 16 rows, or finer when that balances the GPUs), one
// host thread per GPU; the tiles are assembled on the host here (bench.py shows the RCCL gather path used for the
// multi-process launch).  RT_RTRACE_ONE_DEVICE=1 (tests on a one-GPU box): every part renders on device 0.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/rt_host.h"

static std::string fmt_duration(double seconds) {  // Rust `{:.2?}` of a Duration
    char buf[64];
    if (seconds >= 1.0) std::snprintf(buf, sizeof buf, "%.2fs", seconds);
    else if (seconds >= 1e-3) std::snprintf(buf, sizeof buf, "%.2fms", seconds * 1e3);
    else if (seconds >= 1e-6) std::snprintf(buf, sizeof buf, "%.2f\xC2\xB5s", seconds * 1e6);
    else std::snprintf(buf, sizeof buf, "%.2fns", seconds * 1e9);
    return buf;
}

static int fail(const char* msg) {
    std::fprintf(stderr, "Error: %s\n", msg);
    return 1;
}

// One GPU, passes of rth_progressive(host) replicas; returns the process exit status.
static int render_progressive(RtHost* host, const std::function<double()>& since) {
    const RtCameraDesc* cam = rth_camera(host);
    const RtRenderParams* params = rth_params(host);
    const uint32_t W = cam->image_width, H = cam->image_height, T = params->thread_count;
    const bool adaptive = rth_noise_threshold(host) > 0.0;
    RtAdaptiveParams ap;
    rt_adaptive_default_params(&ap);
    if (adaptive) {
        ap.threshold = rth_noise_threshold(host);
        if (rth_adaptive_min(host) >= 0) ap.min_replicas = uint32_t(rth_adaptive_min(host));
        if (rth_adaptive_check(host) >= 0) ap.check_interval = uint32_t(rth_adaptive_check(host));
        if (rth_adaptive_radius(host) >= 0) ap.radius = uint32_t(rth_adaptive_radius(host));
    }
    const uint32_t n = rth_progressive(host) ? rth_progressive(host) : ap.check_interval;
    const std::string ckpt = rth_checkpoint(host);
    const double limit = rth_time_limit(host);
    RtDenoiseParams dp;
    rt_denoise_default_params(&dp);
    dp.iterations = rth_denoise(host);
    std::vector<uint8_t> rgb_dn(dp.iterations ? size_t(W) * H * 3 : 0);
    RtScene* scene = nullptr;
    RtAccum* acc = nullptr;
    if (rt_scene_create(rth_scene(host), 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    if (rt_accum_create(scene, cam, params, &acc) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtAccum, void (*)(RtAccum*)> acc_guard(acc, rt_accum_destroy);
    if (adaptive && rt_accum_set_adaptive(acc, &ap) != RT_OK) return fail(rt_last_error());
    auto save_denoised = [&]() -> bool {  // out_denoised.png from the accumulator's current estimate
        if (!dp.iterations) return true;
        if (rt_accum_preview_denoised_rgb8(acc, &dp, rgb_dn.data()) != RT_OK) { fail(rt_last_error()); return false; }
        if (rth_save_png_rgb8("out_denoised.png", rgb_dn.data(), W, H) != RT_OK) { fail(rth_last_error()); return false; }
        return true;
    };
    std::vector<char> state(rt_accum_state_size(acc));
    if (!ckpt.empty()) {
        std::ifstream in(ckpt, std::ios::binary);
        if (in) {
            std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            if (rt_accum_load_state(acc, blob.data(), blob.size()) != RT_OK) return fail((ckpt + ": " + rt_last_error()).c_str());
            std::printf("Resumed from %s at %u/%u replicas\n", ckpt.c_str(), rt_accum_replicas_done(acc), T);
        }
    }
    auto save = [&]() -> bool {
        if (ckpt.empty()) return true;
        if (rt_accum_save_state(acc, state.data(), state.size()) != RT_OK) { fail(rt_last_error()); return false; }
        const std::string tmp = ckpt + ".tmp";
        std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
        out.write(state.data(), std::streamsize(state.size()));
        out.close();
        if (!out || std::rename(tmp.c_str(), ckpt.c_str()) != 0) { fail(("cannot write " + ckpt).c_str()); return false; }
        return true;
    };
    std::vector<uint8_t> rgb(size_t(W) * H * 3);
    for (uint32_t pass = 1; !rt_accum_finished(acc); pass++) {
        const double ts = since();
        if (rt_accum_render(acc, n, nullptr, nullptr) != RT_OK) return fail(rt_last_error());
        const uint32_t k = rt_accum_replicas_done(acc);
        std::printf("Pass %u: %u/%u replicas in %s\n", pass, k, T, fmt_duration(since() - ts).c_str());
        std::fflush(stdout);
        if (!save()) return 1;
        if (rt_accum_finished(acc)) break;  // the final image goes through the host output stage below
        if (rt_accum_preview_rgb8(acc, rgb.data()) != RT_OK) return fail(rt_last_error());
        if (rth_save_png_rgb8("out.png", rgb.data(), W, H) != RT_OK) return fail(rth_last_error());
        if (!save_denoised()) return 1;
        if (limit >= 0.0 && since() > limit) {
            std::printf("Stopped at %u/%u replicas\n", k, T);
            return 0;
        }
    }
    std::vector<double> frame(size_t(W) * H * 4);
    if (rt_accum_estimate(acc, frame.data()) != RT_OK) return fail(rt_last_error());  // k = T: the frame itself
    std::printf("Done: %s. Writing output to file...\n", fmt_duration(since()).c_str());
    if (rth_save_png("out.png", frame.data(), W, H) != RT_OK) return fail(rth_last_error());
    if (adaptive) {  // where the samples went: n / T in grey
        std::vector<uint32_t> counts(size_t(W) * H);
        if (rt_accum_sample_counts(acc, counts.data()) != RT_OK) return fail(rt_last_error());
        unsigned long long replicas = 0, stopped = 0;
        for (size_t i = 0; i < counts.size(); i++) {
            replicas += counts[i];
            stopped += counts[i] < T ? 1u : 0u;
            const uint8_t g = uint8_t(double(counts[i]) / double(T) * 255.0 + 0.5);
            rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = g;
        }
        if (rth_save_png_rgb8("out_samples.png", rgb.data(), W, H) != RT_OK) return fail(rth_last_error());
        const unsigned long long per_replica = rth_samples_per_pixel(host) / T;  // S^2
        std::printf("Adaptive: %llu/%llu samples rendered, %llu/%llu pixels stopped\n", replicas * per_replica,
                    (unsigned long long)counts.size() * T * per_replica, stopped, (unsigned long long)counts.size());
    }
    if (!save_denoised()) return 1;
    std::printf("Done! Took %s. Goodbye :)\n", fmt_duration(since()).c_str());
    return 0;
}

// --sequence: one device scene, updated in place from one scene file to the next; returns the process exit status.
static int render_sequence(RtHost* host, int argc, char** argv, const std::vector<std::string>& files, const std::function<double()>& since) {
    const RtCameraDesc* cam = rth_camera(host);
    RtScene* scene = nullptr;
    if (rt_scene_create(rth_scene(host), 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    std::vector<double> frame(size_t(cam->image_width) * cam->image_height * 4, 0.0);
    if (rt_render(scene, cam, rth_params(host), frame.data()) != RT_OK) return fail(rt_last_error());
    std::printf("Done: %s. Writing output to file...\n", fmt_duration(since()).c_str());
    if (rth_save_png("out.png", frame.data(), cam->image_width, cam->image_height) != RT_OK) return fail(rth_last_error());
    for (size_t k = 0; k < files.size(); k++) {
        // the same command line with this file as the scene (the last scene name wins)
        std::vector<char*> args(argv, argv + argc);
        std::string name = files[k];
        args.push_back(&name[0]);
        RtHost* next = nullptr;
        if (rth_load(int(args.size()), args.data(), &next) != RT_OK) return fail((files[k] + ": " + rth_last_error()).c_str());
        std::unique_ptr<RtHost, void (*)(RtHost*)> next_guard(next, rth_destroy);
        RtSceneUpdateInfo info;
        if (rt_scene_update(scene, rth_scene(next), &info) != RT_OK) return fail((files[k] + ": " + rt_last_error()).c_str());
        const RtCameraDesc* c = rth_camera(next);
        frame.assign(size_t(c->image_width) * c->image_height * 4, 0.0);
        const double ts = since();
        if (rt_render(scene, c, rth_params(next), frame.data()) != RT_OK) return fail(rt_last_error());
        char out[32];
        std::snprintf(out, sizeof out, "out_%04zu.png", k + 1);
        std::printf("Frame %zu (%s): %u meshes refit, %u triangles, update %s, render %s\n", k + 1, out, info.n_meshes_refit, info.n_triangles_refit,
                    fmt_duration(info.total_ms * 1e-3).c_str(), fmt_duration(since() - ts).c_str());
        std::fflush(stdout);
        if (rth_save_png(out, frame.data(), c->image_width, c->image_height) != RT_OK) return fail(rth_last_error());
    }
    std::printf("Done! Took %s. Goodbye :)\n", fmt_duration(since()).c_str());
    return 0;
}

// --pick: closest hits of the rays through the named pixels' centres, one line each; returns the process exit status.
static int pick_pixels(RtHost* host) {
    const RtCameraDesc* cam = rth_camera(host);
    const RtSceneDesc* desc = rth_scene(host);
    const uint32_t n = rth_pick(host, nullptr, 0);
    std::vector<uint32_t> xy(2 * size_t(n));
    rth_pick(host, xy.data(), n);
    std::vector<double> o(3 * size_t(n)), d(3 * size_t(n));
    for (uint32_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            o[3 * size_t(i) + a] = cam->position[a];
            d[3 * size_t(i) + a] = cam->first_pixel[a] + double(xy[2 * i]) * cam->pixel_delta_u[a] + double(xy[2 * i + 1]) * cam->pixel_delta_v[a] - cam->position[a];
        }
    RtScene* scene = nullptr;
    if (rt_scene_create(desc, 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    std::vector<RtRayHit> hits(n);
    if (rt_trace_rays(scene, n, o.data(), d.data(), rth_params(host)->precision, hits.data()) != RT_OK) return fail(rt_last_error());
    static const char* const kTypes[] = {"?", "sphere", "plane", "mesh", "list", "transform", "bvh", "sky", "sun", "volume", "null"};
    for (uint32_t i = 0; i < n; i++) {
        const RtRayHit& h = hits[i];
        if (!(h.flags & RT_RAY_HIT)) {
            std::printf("Pick %u,%u: miss\n", xy[2 * i], xy[2 * i + 1]);
            continue;
        }
        const uint32_t type = h.node >= 0 && uint32_t(h.node) < desc->n_nodes ? desc->nodes[h.node].type : 0u;
        std::printf("Pick %u,%u: node %d (%s) material %d triangle %d t %.17g position %.17g %.17g %.17g\n", xy[2 * i], xy[2 * i + 1], h.node,
                    type <= 10u ? kTypes[type] : "?", h.material, h.prim, h.t, h.pos[0], h.pos[1], h.pos[2]);
    }
    return 0;
}

// --sh-probe: the nine RGB coefficients of the SH probe at each named position, one line each; returns the process exit status.
static int bake_sh_probes(RtHost* host) {
    const uint32_t n = rth_sh_probes(host, nullptr, 0);
    std::vector<double> pos(3 * size_t(n)), sh(36 * size_t(n));
    rth_sh_probes(host, pos.data(), n);
    RtRenderParams p = *rth_params(host);  // S, T, depth, background, bias, seed, precision of the run; a bake has one scheduler and no partition
    p.pipeline = RT_PIPELINE_AUTO;
    p.collect_stats = 0;
    p.band_rows = p.n_parts = p.part = 0;
    RtScene* scene = nullptr;
    if (rt_scene_create(rth_scene(host), 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    if (rt_bake_probes(scene, n, pos.data(), &p, sh.data()) != RT_OK) return fail(rt_last_error());
    for (uint32_t i = 0; i < n; i++) {
        std::printf("SH probe %u at %.17g %.17g %.17g: %u paths\n", i, pos[3 * size_t(i)], pos[3 * size_t(i) + 1], pos[3 * size_t(i) + 2],
                    p.sqrt_spt * p.sqrt_spt * p.thread_count);
        for (uint32_t k = 0; k < 9; k++) {
            const double* c = &sh[36 * size_t(i) + 4 * k];
            std::printf("SH probe %u coefficient %u: %.17g %.17g %.17g\n", i, k, c[0], c[1], c[2]);
        }
    }
    return 0;
}

// --nearest: the closest surface point of the scene to each listed point, one line each; returns the process exit status.
static int nearest_points(RtHost* host) {
    const uint32_t n = rth_nearest_points(host, nullptr, 0);
    std::vector<double> q(3 * size_t(n));
    rth_nearest_points(host, q.data(), n);
    std::vector<RtPointHit> hits(n);
    RtScene* scene = nullptr;
    if (rt_scene_create(rth_scene(host), 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    if (rt_closest_points(scene, n, q.data(), nullptr, rth_params(host)->precision, hits.data()) != RT_OK) return fail(rt_last_error());
    for (uint32_t i = 0; i < n; i++) {
        const RtPointHit& h = hits[i];
        std::printf("Nearest %u: distance %.17g position %.17g %.17g %.17g normal %.17g %.17g %.17g node %d triangle %d material %d flags %u\n", i,
                    h.distance, h.pos[0], h.pos[1], h.pos[2], h.normal[0], h.normal[1], h.normal[2], h.node, h.prim, h.material, h.flags);
    }
    return 0;
}

// --lightmap: the irradiance map of the k-th mesh op over its own UVs to out_lightmap.png; returns the process exit status.
static int bake_lightmap(RtHost* host, const std::function<double()>& since) {
    uint32_t k = 0, H = 0, passes = 0;
    const uint32_t W = rth_lightmap(host, &k, &H, &passes);
    const RtSceneDesc* desc = rth_scene(host);
    uint32_t n_ops = 0;
    if (rt_scene_op_nodes(desc, nullptr, 0, &n_ops) != RT_OK) return fail(rt_last_error());
    std::vector<int32_t> op_node(n_ops);
    if (rt_scene_op_nodes(desc, op_node.data(), n_ops, &n_ops) != RT_OK) return fail(rt_last_error());
    // the k-th op that came from a mesh node, and which of that node's ops it is
    int32_t node = -1;
    uint32_t instance = 0, seen = 0;
    for (uint32_t pc = 0; pc < n_ops && node < 0; pc++) {
        const int32_t n = op_node[pc];
        if (n < 0 || uint32_t(n) >= desc->n_nodes || desc->nodes[n].type != RT_NODE_MESH) continue;
        if (seen++ != k) continue;
        node = n;
        for (uint32_t q = 0; q < pc; q++)
            if (op_node[q] == n) instance++;
    }
    if (node < 0) return fail(("--lightmap: the scene has " + std::to_string(seen) + " mesh op(s), there is no mesh " + std::to_string(k)).c_str());
    RtRenderParams p = *rth_params(host);  // S, T, depth, background, bias, seed, precision of the run; a bake has one scheduler and no partition
    p.pipeline = RT_PIPELINE_AUTO;
    p.collect_stats = 0;
    p.band_rows = p.n_parts = p.part = 0;
    RtScene* scene = nullptr;
    if (rt_scene_create(desc, 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    const size_t n = size_t(W) * H;
    std::vector<double> rgba(4 * n);
    std::vector<uint8_t> coverage(n);
    if (rt_bake_lightmap(scene, uint32_t(node), instance, W, H, RT_LIGHTMAP_IRRADIANCE, &p, nullptr, int32_t(passes), rgba.data(), coverage.data()) != RT_OK)
        return fail(rt_last_error());
    RtLightmapStats st{};
    rt_lightmap_stats(scene, &st);
    std::printf("Lightmap of mesh %u (node %d): %ux%u texels, %llu covered, %u paths each, %u dilation passes; rasterised in %.3f ms\n", k, node, W, H,
                (unsigned long long)st.covered_texels, p.sqrt_spt * p.sqrt_spt * p.thread_count, passes, st.bin_ms + st.raster_ms);
    std::printf("Done: %s. Writing output to file...\n", fmt_duration(since()).c_str());
    if (rth_save_png("out_lightmap.png", rgba.data(), W, H) != RT_OK) return fail(rth_last_error());
    std::printf("Done! Took %s. Goodbye :)\n", fmt_duration(since()).c_str());
    return 0;
}

// --probe: the panorama at the named point to out_probe.png; returns the process exit status.
static int render_probe(RtHost* host, const std::function<double()>& since) {
    double position[3];
    const uint32_t W = rth_probe(host, position), H = W / 2;
    const size_t n = size_t(W) * H;
    std::vector<double> o(3 * n), d(3 * n), frame(4 * n);
    if (rth_probe_rays(position, W, H, o.data(), d.data()) != RT_OK) return fail(rth_last_error());
    RtScene* scene = nullptr;
    if (rt_scene_create(rth_scene(host), 0, &scene) != RT_OK) return fail(rt_last_error());
    std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
    if (rt_render_rays(scene, n, o.data(), d.data(), rth_params(host), frame.data()) != RT_OK) return fail(rt_last_error());
    std::printf("Probe at %.17g %.17g %.17g: %ux%u texels, no pixel filter (every sample along the texel's centre ray)\n", position[0], position[1],
                position[2], W, H);
    std::printf("Done: %s. Writing output to file...\n", fmt_duration(since()).c_str());
    if (rth_save_png("out_probe.png", frame.data(), W, H) != RT_OK) return fail(rth_last_error());
    std::printf("Done! Took %s. Goodbye :)\n", fmt_duration(since()).c_str());
    return 0;
}

// --ao, --irradiance: the first hits of the --pick ray of every pixel, row-major, as hit records on the device, and room for
// `out_each` bytes of results per pixel.  Everything is freed with the object.
struct PixelHits {
    size_t n = 0;
    void *d_rays = nullptr, *d_hits = nullptr, *d_out = nullptr;
    std::string what;  // the flag, for messages
    ~PixelHits() {
        (void)hipFree(d_rays);
        (void)hipFree(d_hits);
        (void)hipFree(d_out);
    }
    bool hip_ok(hipError_t e, std::string* err) const {
        if (e != hipSuccess) *err = what + ": " + hipGetErrorString(e);
        return e == hipSuccess;
    }
    static bool rt_ok(int st, std::string* err) {
        if (st != RT_OK) *err = rt_last_error();
        return st == RT_OK;
    }
    bool trace(const RtScene* scene, const RtCameraDesc* cam, uint32_t precision, size_t out_each, const char* flag, std::string* err) {
        what = flag;
        const uint32_t W = cam->image_width, H = cam->image_height;
        n = size_t(W) * H;
        std::vector<double> rays(6 * n);  // origins, then directions
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++)
                for (int a = 0; a < 3; a++) {
                    const size_t i = size_t(y) * W + x;
                    rays[3 * i + a] = cam->position[a];
                    rays[3 * (n + i) + a] = cam->first_pixel[a] + double(x) * cam->pixel_delta_u[a] + double(y) * cam->pixel_delta_v[a] - cam->position[a];
                }
        return hip_ok(hipMalloc(&d_rays, rays.size() * sizeof(double)), err) && hip_ok(hipMalloc(&d_hits, n * sizeof(RtRayHit)), err) &&
               hip_ok(hipMalloc(&d_out, n * out_each), err) &&
               hip_ok(hipMemcpy(d_rays, rays.data(), rays.size() * sizeof(double), hipMemcpyHostToDevice), err) &&
               rt_ok(rt_trace_rays_device(scene, n, static_cast<const double*>(d_rays), static_cast<const double*>(d_rays) + 3 * n, precision,
                                          static_cast<RtRayHit*>(d_hits), nullptr), err);
    }
    const RtRayHit* hits() const { return static_cast<const RtRayHit*>(d_hits); }
};

// --ao: visibility of every pixel's first hit (w * h values, row-major; 1 where the pixel sees no surface); false with *err
// set on failure.
static bool bake_ao(const RtScene* scene, const RtCameraDesc* cam, const RtRenderParams* params, uint32_t samples, double max_distance,
                    std::vector<double>* visibility, double* mean_out, std::string* err) {
    PixelHits px;
    RtBakeParams bp{};
    bp.samples = samples;
    bp.precision = params->precision;
    bp.seed = params->seed;
    bp.bias = 0.001;
    bp.max_distance = max_distance;
    if (!px.trace(scene, cam, params->precision, sizeof(RtBakeResult), "--ao", err)) return false;
    const size_t n = px.n;
    std::vector<RtBakeResult> out(n);
    if (!PixelHits::rt_ok(rt_bake_visibility_hits_device(scene, n, px.hits(), &bp, static_cast<RtBakeResult*>(px.d_out), nullptr), err) ||
        !px.hip_ok(hipMemcpy(out.data(), px.d_out, n * sizeof(RtBakeResult), hipMemcpyDeviceToHost), err))
        return false;
    visibility->resize(n);
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) {
        (*visibility)[i] = out[i].visibility;
        sum += out[i].visibility;
    }
    *mean_out = n ? sum / double(n) : 0.0;
    return true;
}

// --irradiance: the bake at every pixel's first hit (w * h x 4 values, row-major; 0 where the pixel sees no surface); false with
// *err set on failure.
static bool bake_irradiance(const RtScene* scene, const RtCameraDesc* cam, const RtRenderParams* params, std::vector<double>* rgba, double* mean_out,
                            std::string* err) {
    PixelHits px;
    RtRenderParams bp = *params;  // S, T, depth, background, bias, seed, precision of the run; the bake has one scheduler and no partition
    bp.pipeline = RT_PIPELINE_AUTO;
    bp.collect_stats = 0;
    bp.band_rows = bp.n_parts = bp.part = 0;
    if (!px.trace(scene, cam, params->precision, 4 * sizeof(double), "--irradiance", err)) return false;
    const size_t n = px.n;
    rgba->assign(4 * n, 0.0);
    if (!PixelHits::rt_ok(rt_bake_irradiance_hits_device(scene, n, px.hits(), &bp, static_cast<double*>(px.d_out), nullptr), err) ||
        !px.hip_ok(hipMemcpy(rgba->data(), px.d_out, 4 * n * sizeof(double), hipMemcpyDeviceToHost), err))
        return false;
    double sum = 0.0;  // mean luminance over the finite pixels, as the light groups report theirs
    size_t finite = 0;
    for (size_t i = 0; i < n; i++) {
        const double y = (0.2126 * (*rgba)[4 * i] + 0.7152 * (*rgba)[4 * i + 1]) + 0.0722 * (*rgba)[4 * i + 2];
        if (y - y == 0.0) { sum += y; finite++; }
    }
    *mean_out = finite ? sum / double(finite) : 0.0;
    return true;
}

int main(int argc, char** argv) {
    using clock = std::chrono::steady_clock;
    auto t0 = clock::now();
    auto since = [&]() { return std::chrono::duration<double>(clock::now() - t0).count(); };
    std::vector<std::string> sequence;  // --sequence=<scene1>[,<scene2>...] (the scene loader ignores the flag)
    for (int i = 1; i < argc; i++)
        if (!std::strncmp(argv[i], "--sequence=", 11)) {
            std::string rest = argv[i] + 11;
            for (size_t at = 0; at <= rest.size();) {
                const size_t comma = std::min(rest.find(',', at), rest.size());
                if (comma > at) sequence.push_back(rest.substr(at, comma - at));
                at = comma + 1;
            }
        }

    RtHost* host = nullptr;
    if (rth_load(argc, argv, &host) != RT_OK) {
        std::fprintf(stderr, "Error: %s\n", rth_last_error());
        return 1;
    }
    std::fputs(rth_log(host), stdout);  // "Loaded N tris", loader warnings
    const RtCameraDesc* cam = rth_camera(host);
    const RtRenderParams* params = rth_params(host);
    std::printf("Ready: %s\n", fmt_duration(since()).c_str());  // main.rs:62
    uint32_t spp = rth_samples_per_pixel(host);
    std::printf("Rendering: %ux%u @%uspp on %u threads (%u samples/thread)\n", cam->image_width, cam->image_height, spp,
                params->thread_count, spp / params->thread_count);  // main.rs:68-71
    std::fflush(stdout);

    if (rth_sh_probes(host, nullptr, 0) != 0) {  // refused BEFORE a device is touched
        if (!sequence.empty()) return fail("--sh-probe bakes probes instead of the frame: it cannot be combined with --sequence");
        if (params->max_depth == 0) return fail("--sh-probe needs a depth of at least 1");
    }
    if (rth_nearest_points(host, nullptr, 0) != 0 && !sequence.empty())
        return fail("--nearest queries points instead of rendering the frame: it cannot be combined with --sequence");
    if (rth_lightmap(host, nullptr, nullptr, nullptr) != 0) {  // refused BEFORE a device is touched
        if (!sequence.empty()) return fail("--lightmap bakes a lightmap instead of the frame: it cannot be combined with --sequence");
        if (params->max_depth == 0) return fail("--lightmap needs a depth of at least 1");
    }
    uint32_t gpus = rth_gpus(host);
    int available = rt_device_count();
    if (available < 1) {
        std::fprintf(stderr, "Error: no HIP device (the render path has no CPU fallback)\n");
        return 1;
    }
    if (rth_pick(host, nullptr, 0) != 0) {
        const int rc = pick_pixels(host);
        rth_destroy(host);
        return rc;
    }
    if (rth_sh_probes(host, nullptr, 0) != 0) {
        const int rc = bake_sh_probes(host);
        rth_destroy(host);
        return rc;
    }
    if (rth_nearest_points(host, nullptr, 0) != 0) {
        const int rc = nearest_points(host);
        rth_destroy(host);
        return rc;
    }
    if (rth_lightmap(host, nullptr, nullptr, nullptr) != 0) {
        const int rc = bake_lightmap(host, since);
        rth_destroy(host);
        return rc;
    }
    if (rth_probe(host, nullptr) != 0) {
        if (!sequence.empty()) return fail("--probe renders a panorama instead of the frame: it cannot be combined with --sequence");
        const int rc = render_probe(host, since);
        rth_destroy(host);
        return rc;
    }
    if (!sequence.empty()) {
        if (gpus > 1 || rth_progressive(host) || rth_noise_threshold(host) > 0.0 || rth_light_groups(host) || rth_denoise(host) || rth_ao(host, nullptr) ||
            rth_irradiance(host))
            return fail("--sequence renders whole frames on one GPU: it cannot be combined with --gpus > 1, --progressive, --noise-threshold, "
                        "--light-groups, --denoise, --ao or --irradiance");
        const int rc = render_sequence(host, argc, argv, sequence, since);
        rth_destroy(host);
        return rc;
    }
    if (rth_progressive(host) || rth_noise_threshold(host) > 0.0) {
        const int rc = render_progressive(host, since);
        rth_destroy(host);
        return rc;
    }
    const char* one_dev = std::getenv("RT_RTRACE_ONE_DEVICE");
    const bool rehearsal = one_dev && std::atoi(one_dev) != 0;
    if (!rehearsal && int(gpus) > available) gpus = uint32_t(available);
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint32_t band = gpus > 1 ? rth_band_rows(H, gpus) : 16;  // interleaved row bands
    std::vector<double> frame(size_t(W) * H * 4, 0.0);  // camera.create_buffer(), main.rs:74
    const uint32_t denoise = rth_denoise(host);         // one GPU (rth_load refuses --denoise with --gpus > 1)
    std::vector<double> denoised(denoise ? frame.size() : 0);
    // light groups: one GPU, whole frames (rth_load refuses the other combinations)
    const uint32_t max_groups = rth_light_groups(host);
    const RtSceneDesc* desc = rth_scene(host);
    std::vector<uint8_t> material_group(max_groups ? desc->n_materials : 0);
    RtLightGroups lg{};
    std::vector<double> group_frames, mixed;
    if (max_groups) {
        if (rt_light_groups_auto(desc, max_groups, int(params->has_background), material_group.data(), &lg.background_group, &lg.n_groups) != RT_OK)
            return fail(rt_last_error());
        lg.n_materials = desc->n_materials;
        lg.material_group = material_group.data();
        lg.unlit_group = 0;
        group_frames.resize(frame.size() * lg.n_groups);
    }
    double ao_distance = 0.0;
    const uint32_t ao_samples = rth_ao(host, &ao_distance);  // one GPU (rth_load refuses --ao with --gpus > 1)
    if (ao_samples) {  // refused BEFORE the render: a bake that fails afterwards would throw the frame away
        uint32_t info = 0;
        if (rt_scene_info(rth_scene(host), &info) != RT_OK) return fail(rt_last_error());
        if (info & RT_SCENE_INFO_VOLUMES) return fail("--ao does not support scenes with volumes (a medium gives no deterministic surface)");
    }
    const bool irradiance = rth_irradiance(host) != 0;  // one GPU (rth_load refuses --irradiance with --gpus > 1)
    if (irradiance) {  // refused BEFORE the render, like --ao's
        uint32_t info = 0;
        if (rt_scene_info(rth_scene(host), &info) != RT_OK) return fail(rt_last_error());
        if (info & RT_SCENE_INFO_VOLUMES) return fail("--irradiance does not support scenes with volumes (the ray queries that find the surface points have none)");
        if (params->max_depth == 0) return fail("--irradiance needs a depth of at least 1");
    }
    std::vector<double> irr_rgba;
    double irr_mean = 0.0, irr_seconds = 0.0;
    std::vector<double> ao_visibility;
    double ao_mean = 0.0, ao_seconds = 0.0;
    std::vector<std::string> errors(gpus);
    std::vector<std::thread> workers;
    for (uint32_t g = 0; g < gpus; g++) {
        workers.emplace_back([&, g]() {
            auto tg = clock::now();
            RtScene* scene = nullptr;
            if (rt_scene_create(rth_scene(host), rehearsal ? 0 : int(g), &scene) != RT_OK) {
                errors[g] = rt_last_error();
                return;
            }
            RtRenderParams p = *params;
            if (gpus > 1) {
                p.band_rows = band;
                p.n_parts = gpus;
                p.part = g;
            }
            uint32_t rows = rt_owned_rows(H, &p);
            std::vector<double> part(size_t(rows) * W * 4);
            std::unique_ptr<RtScene, void (*)(RtScene*)> scene_guard(scene, rt_scene_destroy);
            if (max_groups) {  // the group frames and the frame itself from one render
                if (rt_render_light_groups(scene, cam, &p, &lg, group_frames.data(), part.data()) != RT_OK) errors[g] = rt_last_error();
            } else if (rows && rt_render(scene, cam, &p, part.data()) != RT_OK) errors[g] = rt_last_error();
            if (!errors[g].empty()) return;
            uint32_t r = 0;
            for (uint32_t y = 0; y < H; y++) {
                bool mine = gpus == 1 || (y / band) % gpus == g;
                if (!mine) continue;
                std::memcpy(&frame[size_t(y) * W * 4], &part[size_t(r) * W * 4], size_t(W) * 4 * sizeof(double));
                r++;
            }
            // the reference prints one line per render thread (camera.rs:236); here: one per GPU
            std::printf("GPU %u finished in %s\n", g, fmt_duration(std::chrono::duration<double>(clock::now() - tg).count()).c_str());
            std::fflush(stdout);
            double weights[RT_LIGHT_GROUPS_MAX];
            const int32_t n_weights = max_groups ? rth_light_mix(host, weights, RT_LIGHT_GROUPS_MAX) : -1;
            if (n_weights >= 0) {
                double tints[3 * RT_LIGHT_GROUPS_MAX];
                for (uint32_t k = 0; k < lg.n_groups; k++) tints[3 * k] = tints[3 * k + 1] = tints[3 * k + 2] = int32_t(k) < n_weights ? weights[k] : 1.0;
                mixed.resize(frame.size());
                if (rt_light_mix(rehearsal ? 0 : int(g), group_frames.data(), lg.n_groups, W, H, tints, mixed.data()) != RT_OK) errors[g] = rt_last_error();
            }
            if (denoise) {  // the whole frame: gpus == 1
                RtDenoiseParams dp;
                rt_denoise_default_params(&dp);
                dp.iterations = denoise;
                std::vector<double> aov(size_t(W) * H * 8);
                if (rt_render_aov(scene, cam, &p, dp.aov_replicas, aov.data()) != RT_OK ||
                    rt_denoise(rehearsal ? 0 : int(g), frame.data(), aov.data(), W, H, &dp, denoised.data()) != RT_OK)
                    errors[g] = rt_last_error();
            }
            if (ao_samples && errors[g].empty()) {
                auto ta = clock::now();
                if (!bake_ao(scene, cam, &p, ao_samples, ao_distance, &ao_visibility, &ao_mean, &errors[g])) return;
                ao_seconds = std::chrono::duration<double>(clock::now() - ta).count();
            }
            if (irradiance && errors[g].empty()) {
                auto ta = clock::now();
                if (!bake_irradiance(scene, cam, &p, &irr_rgba, &irr_mean, &errors[g])) return;
                irr_seconds = std::chrono::duration<double>(clock::now() - ta).count();
            }
        });
    }
    for (auto& t : workers) t.join();
    for (auto& e : errors)
        if (!e.empty()) {
            std::fprintf(stderr, "Error: %s\n", e.c_str());
            return 1;
        }
    for (uint32_t k = 0; k < (max_groups ? lg.n_groups : 0u); k++) {  // id, what it holds, mean luminance over the finite pixels
        std::string holds = k == 0 ? "unlit" : "";
        for (uint32_t m = 0; m < lg.n_materials; m++)
            if (material_group[m] == k && desc->materials[m].type == RT_MAT_EMISSIVE) holds += (holds.empty() ? "material " : ", material ") + std::to_string(m);
        if (params->has_background && lg.background_group == k) holds += holds.empty() ? "background" : ", background";
        const double* f = &group_frames[size_t(k) * frame.size()];
        double sum = 0.0;
        size_t finite = 0;
        for (size_t i = 0; i < size_t(W) * H; i++) {
            const double y = (0.2126 * f[4 * i] + 0.7152 * f[4 * i + 1]) + 0.0722 * f[4 * i + 2];
            if (y - y == 0.0) { sum += y; finite++; }
        }
        std::printf("Light group %u: %s, mean luminance %.6g\n", k, holds.c_str(), finite ? sum / double(finite) : 0.0);
    }
    std::printf("Done: %s. Writing output to file...\n", fmt_duration(since()).c_str());  // main.rs:78
    if (rth_save_png("out.png", frame.data(), W, H) != RT_OK) {                           // main.rs:23,80-82
        std::fprintf(stderr, "Error: %s\n", rth_last_error());
        return 1;
    }
    for (uint32_t k = 0; k < (max_groups ? lg.n_groups : 0u); k++)
        if (rth_save_png(("out_light_" + std::to_string(k) + ".png").c_str(), &group_frames[size_t(k) * frame.size()], W, H) != RT_OK) return fail(rth_last_error());
    if (!mixed.empty() && rth_save_png("out_mixed.png", mixed.data(), W, H) != RT_OK) return fail(rth_last_error());
    if (ao_samples) {
        if (rth_save_png_grey("out_ao.png", ao_visibility.data(), W, H) != RT_OK) return fail(rth_last_error());
        std::printf("Ambient occlusion: %u samples per pixel, mean visibility %.6g, baked in %s\n", ao_samples, ao_mean, fmt_duration(ao_seconds).c_str());
    }
    if (irradiance) {
        if (rth_save_png("out_irradiance.png", irr_rgba.data(), W, H) != RT_OK) return fail(rth_last_error());
        std::printf("Irradiance: %u paths per pixel, mean luminance of the cosine-weighted incoming radiance %.6g, baked in %s\n", spp, irr_mean,
                    fmt_duration(irr_seconds).c_str());
    }
    if (denoise && rth_save_png("out_denoised.png", denoised.data(), W, H) != RT_OK) {
        std::fprintf(stderr, "Error: %s\n", rth_last_error());
        return 1;
    }
    std::printf("Done! Took %s. Goodbye :)\n", fmt_duration(since()).c_str());  // main.rs:85
    rth_destroy(host);
    return 0;
}
