// Internal declarations shared by the host-side translation units.
#pragma once
#include <cmath>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/rt_host.h"
#include "hmath.h"
#include "scene_builder.h"

namespace rth {

// reference src/config.rs:8-18
struct SceneConfig {
    std::optional<size_t> output_width;
    std::optional<double> aspect_ratio, focal_length, f_number, focus_distance;
    std::optional<V4> camera_pos, camera_target, background;
};
SceneConfig default_scene_config();                                    // config.rs:20-29
SceneConfig merge(const SceneConfig& base, const SceneConfig& over);   // config.rs:32-43

// reference src/config.rs:46-59 (+ the new keys)
struct Config {
    SceneConfig scene;
    size_t thread_count = 1;
    size_t sqrt_samples_per_thread = 15;
    size_t max_depth = 20;
    double light_bias = 0.25;
    std::string scene_name;
    // additions
    uint64_t seed = 1;
    uint32_t gpus = 1;
    uint32_t precision = RT_PRECISION_F64;
    uint32_t pipeline = RT_PIPELINE_AUTO;
    bool bvh_on_device = false;  // --bvh=device: RT_SCENE_BVH_ON_DEVICE
    uint32_t progressive = 0;    // --progressive=<n>: passes of n replicas (0: one-shot render)
    std::string checkpoint;      // --checkpoint=<file>: state saved after every pass, resumed from at start-up
    double time_limit = -1.0;    // --time-limit=<seconds>: stop after the first pass that ends past it (< 0: none)
    uint32_t denoise = 0;        // --denoise=<iterations>: also write out_denoised.png (0: off)
    uint32_t light_groups = 0;   // --light-groups[=<max>]: also write out_light_<g>.png (0: off)
    bool has_light_mix = false;  // --light-mix=<w0>,<w1>,...: also write out_mixed.png
    std::vector<double> light_mix;
    double noise_threshold = 0.0;  // --noise-threshold=<x>: adaptive sampling (rt_accum_set_adaptive; 0: off)
    int32_t adaptive_min = -1;     // --adaptive-min=<k>, --adaptive-check=<m>, --adaptive-radius=<r>: -1 = the library's default
    int32_t adaptive_check = -1;
    int32_t adaptive_radius = -1;
    std::vector<std::pair<uint32_t, uint32_t>> pick;  // --pick=<x>,<y>[:<x>,<y>...]: pixels to query instead of rendering
    uint32_t ao_samples = 0;                          // --ao=<samples>[:<max_distance>]: also write out_ao.png (0: off)
    double ao_max_distance = HUGE_VAL;                // +inf: unlimited
    bool irradiance = false;                          // --irradiance: also write out_irradiance.png (rt_bake_irradiance_hits_device)
    bool has_probe = false;                           // --probe=<x>,<y>,<z>[:<width>]: a light probe panorama instead of the frame
    double probe_position[3] = {0.0, 0.0, 0.0};
    uint32_t probe_width = 512;                       // height = width / 2
    std::vector<double> nearest;                      // --nearest=<x>,<y>,<z>[:<x>,<y>,<z>...]: 3 doubles per point, queried instead of rendering
    std::vector<double> sh_probes;                    // --sh-probe=<x>,<y>,<z>[:<x>,<y>,<z>...]: 3 doubles per probe, baked instead of rendering
    bool has_lightmap = false;                        // --lightmap=<k>:<width>[x<height>][:<passes>]: the irradiance map of the k-th mesh op instead of the frame
    uint32_t lightmap_op = 0, lightmap_width = 0, lightmap_height = 0;
    uint32_t lightmap_passes = 2;                     // dilation passes
};
bool config_from_args(int argc, const char* const* argv, Config* out, std::string* err);  // config.rs:62-176

bool parse_f64(const std::string& s, double* out);        // str::parse::<f64>
bool parse_usize(const std::string& s, size_t* out);      // str::parse::<usize>
bool parse_vec3(const std::string& s, double out[3], std::string* err);  // utils.rs:39-50
// `^([^=\s]+)=([^=\s]+)$` (config.rs:63 without the leading '-', loaders/scene.rs:756)
bool split_key_value(const std::string& s, std::string* key, std::string* value);

void make_camera(const SceneConfig& sc, RtCameraDesc* out);  // camera.rs:47-130

// texture/image.rs + buffer.rs:30-48 (PNG, baseline JPEG -> RGB f32)
bool load_image_rgb32f(const std::string& path, std::vector<float>* rgb, uint32_t* width, uint32_t* height, std::string* err);

std::unique_ptr<MeshData> load_obj(const std::string& path, std::string* log, std::string* err);

struct LoadedScene {
    SceneBuilder builder;
    int world = -1, lights = -1;
    SceneConfig scene_config;  // scene-level defaults (@config / hard-coded), before the CLI merge
};
// loaders/scene.rs:80-156
bool load_dsl_scene(const std::string& file_path, const std::string& asset_path, SceneRng& rng,
                    LoadedScene* out, std::string* log, std::string* err);
// scene/golden_monkey.rs:23-139
bool load_default_scene(SceneRng& rng, LoadedScene* out, std::string* log, std::string* err);

void tonemap_rgb8(const double* rgba, uint32_t w, uint32_t h, uint8_t* rgb);  // output.rs + aces.rs
void grey_rgb8(const double* values, uint32_t w, uint32_t h, uint8_t* rgb);   // the sRGB curve of tonemap_rgb8 alone, no ACES
bool write_png_rgb8(const std::string& path, const uint8_t* rgb, uint32_t w, uint32_t h, std::string* err);

}  // namespace rth

struct RtHost {
    rth::Config config;
    rth::LoadedScene scene;
    const RtSceneDesc* desc = nullptr;
    RtCameraDesc camera{};
    RtRenderParams params{};
    std::string log;
};
