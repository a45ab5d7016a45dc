/*
 * rt_host.h — C ABI of the host side that stays *around* the render path
 * (librt_host.so, CPU only, no HIP): the reference's CLI flag parser, scene
 * DSL loader, OBJ loader, default scene, camera set-up and the output stage,
 * restated in C++ because no Rust toolchain exists in the build image.
 *
 *   rth_load        = reference src/main.rs:26-59  (Config::from_args + scene dispatch
 *                     + SceneLoader::load / GoldenMonkeyScene::init + Camera::new)
 *   rth_scene/...   = the flattened `(Camera, world, lights)` SceneData (src/scene.rs:30)
 *                     in the form rt_mi355.h takes
 *   rth_tonemap_rgb8, rth_save_png = Writer::save with tonemap_aces
 *                     (src/output.rs:23-49, src/tonemapping/aces.rs:27-33, main.rs:80-82)
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include "rt_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtHost RtHost;

/* argv[0] is skipped like env::args().skip(1) (config.rs:81).  Flags are the
 * reference's (README.md:21-43) plus --seed=<u64>, --gpus=<n>,
 * --precision=f64|f32, --pipeline=auto|mega|wavefront, --bvh=host|device, --progressive=<n>,
 * --checkpoint=<file>, --time-limit=<seconds>, --denoise=<iterations>, --noise-threshold=<x>,
 * --adaptive-min=<k>, --adaptive-check=<m>, --adaptive-radius=<r>, --light-groups[=<max>],
 * --light-mix=<w0>,<w1>,..., --pick=<x>,<y>[:...], --ao=<samples>[:<max_distance>], --probe=<x>,<y>,<z>[:<width>], --irradiance,
 * --sh-probe=<x>,<y>,<z>[:<x>,<y>,<z>...]
 * --nearest=<x>,<y>,<z>[:<x>,<y>,<z>...]
 * --lightmap=<k>:<width>[x<height>][:<passes>]
 * (unknown keys are ignored by the reference, config.rs:146, so these
 * are compatible).
 * Relative scene/asset paths resolve against the current directory, as in
 * the reference (main.rs:43, golden_monkey.rs:77). */
int rth_load(int argc, const char* const* argv, RtHost** out);
void rth_destroy(RtHost* host);

const RtSceneDesc* rth_scene(const RtHost* host);
const RtCameraDesc* rth_camera(const RtHost* host);
const RtRenderParams* rth_params(const RtHost* host);
uint32_t rth_gpus(const RtHost* host);            /* --gpus, default 1 */
/* Progressive rendering (rt_accum_*): --progressive=<n> replicas per pass (0 = off), --checkpoint=<file> ("" = none),
 * --time-limit=<seconds> (< 0 = none).  rth_load rejects n = 0, --checkpoint without --progressive, --time-limit without
 * --checkpoint and --progressive with --gpus > 1. */
uint32_t rth_progressive(const RtHost* host);
const char* rth_checkpoint(const RtHost* host);
double rth_time_limit(const RtHost* host);
/* --denoise=<iterations> (1 .. RT_DENOISE_MAX_ITERATIONS; 0 = off): rtrace also writes out_denoised.png, the frame (or,
 * with --progressive, the estimate after every pass) filtered by rt_denoise with its first-hit AOVs.  rth_load rejects
 * --denoise with --gpus > 1. */
uint32_t rth_denoise(const RtHost* host);
/* Light groups (rt_render_light_groups with rt_light_groups_auto): --light-groups[=<max>] (1 .. RT_LIGHT_GROUPS_MAX, the
 * bare flag = RT_LIGHT_GROUPS_MAX; 0 = off): rtrace also writes out_light_<g>.png per group and one console line each.
 * --light-mix=<w0>,<w1>,... (finite numbers, at most RT_LIGHT_GROUPS_MAX; groups without an entry weigh 1) also writes
 * out_mixed.png.  rth_light_mix copies up to `capacity` weights and returns how many were given, -1 without the flag.
 * rth_load rejects --light-mix without --light-groups, and --light-groups with --gpus > 1, --progressive,
 * --noise-threshold or --pipeline=mega. */
uint32_t rth_light_groups(const RtHost* host);
int32_t rth_light_mix(const RtHost* host, double* weights_out, uint32_t capacity);
/* Adaptive sampling (rt_accum_set_adaptive): --noise-threshold=<x> (> 0; 0 = off) turns it on and implies passes (of
 * --progressive=<n> replicas if given, else of check_interval); --adaptive-min=<k> (>= 2), --adaptive-check=<m> (>= 1),
 * --adaptive-radius=<r> (0 .. 4): -1 = not given, the library's default.  rth_load rejects values outside these ranges,
 * the three without --noise-threshold, and --noise-threshold with --gpus > 1 or --pipeline=mega. */
double rth_noise_threshold(const RtHost* host);
int32_t rth_adaptive_min(const RtHost* host);
int32_t rth_adaptive_check(const RtHost* host);
int32_t rth_adaptive_radius(const RtHost* host);
/* Ray queries (rt_trace_rays): --pick=<x>,<y>[:<x>,<y>...] names pixels; rtrace then casts the ray through the centre of each
 * (first_pixel + x * pixel_delta_u + y * pixel_delta_v - position from position: no lens, no jitter) and prints one line per
 * pixel - node, node type, material, triangle, t, position - INSTEAD of rendering.  rth_load rejects malformed lists and
 * pixels outside the frame.  rth_pick copies up to `capacity` (x, y) pairs and returns how many were given (0: no flag). */
uint32_t rth_pick(const RtHost* host, uint32_t* xy_out, uint32_t capacity);
/* Ambient occlusion (rt_bake_visibility_hits_device): --ao=<samples>[:<max_distance>] (1 .. 4096 samples; a distance > 0,
 * default unlimited): after the render rtrace casts the --pick ray of every pixel (rt_trace_rays_device), bakes the
 * visibility of every first hit with the run's seed and also writes out_ao.png, grey = visibility through the sRGB curve
 * (no ACES); the hit records stay on the device.  rth_load rejects malformed values, and --ao with --gpus > 1,
 * --progressive, --noise-threshold or --pick; rtrace refuses a scene with volumes before it renders anything.  rth_ao returns the samples (0: no flag) and the distance (+inf: unlimited). */
uint32_t rth_ao(const RtHost* host, double* max_distance_out);
/* Irradiance bake (rt_bake_irradiance_hits_device): --irradiance (no value): rtrace also writes out_irradiance.png, the
 * cosine-weighted mean of the radiance arriving at the first hit of the ray through every pixel's centre (the --pick ray),
 * with the run's -s, -t, depth, bias, seed and precision, through the output stage of out.png; a pixel that sees no surface is
 * black; the hit records stay on the device.  rth_load rejects --irradiance with --gpus > 1, --progressive, --noise-threshold,
 * --pick, --ao or --probe; rtrace refuses a scene with volumes (the ray queries have none) and --sequence before it renders
 * anything.  rth_irradiance returns 1 with the flag, 0 without.                                                              */
int rth_irradiance(const RtHost* host);
/* SH radiance probes (rt_bake_probes): --sh-probe=<x>,<y>,<z>[:<x>,<y>,<z>...] (finite positions): rtrace renders nothing and
 * prints the nine RGB coefficients of every probe, baked with the run's -s, -t, depth, bias, seed and precision, the way --pick
 * prints its hits.  rth_load rejects malformed values, and --sh-probe with --gpus > 1, --progressive, --noise-threshold, --pick,
 * --ao, --probe, --irradiance or --pipeline=mega; rtrace refuses --sequence and a depth of 0 before a device is touched.
 * rth_sh_probes returns the number of probes and writes up to `capacity` positions (3 doubles each; positions_out may be NULL). */
uint32_t rth_sh_probes(const RtHost* host, double* positions_out, uint32_t capacity);
/* Point queries (rt_closest_points): --nearest=<x>,<y>,<z>[:<x>,<y>,<z>...] (finite numbers): rtrace renders nothing and prints, per
 * point, the distance, position and normal of the closest surface point (%.17g each), then node, triangle, material and flags.
 * rth_load rejects malformed values, and --nearest in the combinations --sh-probe is rejected in, and with --sh-probe itself.
 * rth_nearest_points returns the number of points and writes up to `capacity` of them (3 doubles each; points_out may be NULL). */
uint32_t rth_nearest_points(const RtHost* host, double* points_out, uint32_t capacity);
/* Lightmaps (rt_bake_lightmap): --lightmap=<k>:<width>[x<height>][:<passes>] (k: the k-th mesh op of the compiled program,
 * from 0; sizes 1 .. 16384, height = width if not given; dilation passes, default 2, at most 1024): rtrace bakes the
 * irradiance map of that mesh over its own UVs with the run's -s, -t, depth, bias, seed and precision and writes
 * out_lightmap.png, through the output stage of out.png, INSTEAD of the frame; row 0 of the file is v near 0, so the file can
 * be fed back as an image texture.  rth_load rejects malformed values, and --lightmap in the combinations --sh-probe is
 * rejected in, and with --sh-probe or --nearest; rtrace refuses --sequence and a depth of 0 before a device is touched.
 * rth_lightmap returns the width (0: no flag) and copies k, the height and the passes (each pointer may be NULL).            */
uint32_t rth_lightmap(const RtHost* host, uint32_t* op_out, uint32_t* height_out, uint32_t* passes_out);
/* Light probe (rt_render_rays): --probe=<x>,<y>,<z>[:<width>] (a finite position; width 2 .. 65536, default 512; the height
 * is width / 2): rtrace renders the equirectangular panorama of rth_probe_rays at that point with the run's -s, -t, depth,
 * bias, seed and precision and writes out_probe.png INSTEAD of the frame.  No pixel filter: every sample of a texel goes along
 * its centre ray.  rth_load rejects malformed values, and --probe with --gpus > 1, --progressive, --noise-threshold, --pick,
 * --ao, --light-groups, --denoise or --pipeline=mega.  rth_probe returns the width (0: no flag) and copies the position. */
uint32_t rth_probe(const RtHost* host, double position_out[3]);
/* The rays of an equirectangular light probe at `position`, +y up: width * height origins (= position) and directions,
 * 3 doubles each, row-major with row 0 at the top.  Pixel (x, y): phi = ((2 pi) (x + 0.5)) / width - pi,
 * theta = (pi (y + 0.5)) / height, direction = (sin theta sin phi, cos theta, -(sin theta cos phi)) with det_sin / det_cos
 * of rt_detmath.h; f64, every operation rounded once, in this order.  The centre column looks along -z. */
int rth_probe_rays(const double position[3], uint32_t width, uint32_t height, double* origins_out, double* dirs_out);
uint32_t rth_samples_per_pixel(const RtHost* host); /* Camera::samples_per_pixel() */
/* Row partition of `rtrace --gpus=N` (replaces the per-thread full-frame buffers of src/camera.rs:243-255): band height
 * for `height` image rows over `n_parts` GPUs = the largest of 16, 8, 4, 2, 1 rows that gives the most loaded part as few
 * rows as any of them does (the slowest GPU sets the time of the frame); 0 for n_parts <= 1.  The ONE definition of the
 * rule on the native side; rust_raytracer_amd/dist.py (band_rows_for) is its Python twin and a test compares the two. */
uint32_t rth_band_rows(uint32_t height, uint32_t n_parts);
/* Everything the reference would have printed while loading ("Loaded N tris",
 * loader warnings), newline separated. */
const char* rth_log(const RtHost* host);

/* Camera::new + init for explicit settings (used by tests of camera.rs:47-130).
 * f_number / focus_distance < 0 mean None. */
int rth_make_camera(uint32_t width, double aspect_ratio, double focal_length,
                    double f_number, double focus_distance,
                    const double position[3], const double look_at[3],
                    RtCameraDesc* out);

/* ACES fit + sRGB OETF + `(x * 255.999) as u8` on w*h RGBA f64 pixels -> w*h*3 bytes. */
int rth_tonemap_rgb8(const double* rgba, uint32_t w, uint32_t h, uint8_t* rgb_out);
/* The same followed by an 8-bit RGB PNG file (zlib deflate). */
int rth_save_png(const char* path, const double* rgba, uint32_t w, uint32_t h);
/* An 8-bit RGB PNG file of w*h values that are no radiance (rtrace --ao: visibilities in [0, 1]): grey = the value through
 * the clamp, sRGB OETF and quantisation of rth_save_png, WITHOUT the ACES fit. */
int rth_save_png_grey(const char* path, const double* values, uint32_t w, uint32_t h);
/* An 8-bit RGB PNG file of w*h*3 bytes that are already tone-mapped (rt_accum_preview_rgb8). */
int rth_save_png_rgb8(const char* path, const uint8_t* rgb, uint32_t w, uint32_t h);

/* Buffer::from_image (src/buffer.rs:30-48): decodes a PNG or baseline-JPEG file into w*h RGB f32
 * triples (8-bit: x/255, 16-bit: x/65535), row 0 first.  The caller frees with rth_free_image. */
int rth_load_image(const char* path, float** rgb_out, uint32_t* w_out, uint32_t* h_out);
void rth_free_image(float* rgb);

const char* rth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HOST_H */
