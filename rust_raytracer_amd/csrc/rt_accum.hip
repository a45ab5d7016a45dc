// rt_accum.hip — the progressive accumulator (RtAccum, include/rt_mi355.h; DESIGN.md sections 9 to 11): its kernels, the
// adaptive decision step, the state blob, the previews and the denoised previews.  A client of the renderer: it renders
// through rt_render.h and sees a scene through that header's accessors only; its host arithmetic is rt_accum_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "rt_accum_state.h"
#include "rt_aov.h"
#include "rt_desc.h"
#include "rt_device.h"
#include "rt_owned.h"
#include "rt_render.h"

// ---------------------------------------------------------------------------------------------
// Progressive rendering (RtAccum, include/rt_mi355.h): estimate scaling, device output stage
// ---------------------------------------------------------------------------------------------
namespace rt {

// estimate = sum_k * (T / k), every double of the (owned_rows x width x 4) layout (w stays 0)
__global__ void __launch_bounds__(256) k_accum_estimate(const double* __restrict__ sum, uint64_t n, double scale, double* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sum[i] * scale;
}

// The host output stage (csrc/host/output.cpp tonemap_rgb8: ACES fit, clamp, sRGB OETF, saturating u8) on the device,
// operation for operation and without contraction (the host build never fuses a*b+c); only pow may differ from the host's
// in the last bit.  Input pixel i is rgba[4 i ..] * scale: the estimate of an accumulator is tone-mapped without a second
// pass over HBM (scale 1 for a plain frame: x * 1 == x, and a NaN maps to 0 whatever its payload).
__global__ void __launch_bounds__(256) k_tonemap_rgb8(const double* __restrict__ rgba, uint64_t npix, double scale, uint8_t* __restrict__ rgb) {
#pragma clang fp contract(off)
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double kIn[9] = {0.59719, 0.35458, 0.04823, 0.07600, 0.90834, 0.01566, 0.02840, 0.13383, 0.83777};
    const double kOut[9] = {1.60475, -0.53108, -0.07367, -0.10208, 1.10813, -0.00605, -0.00327, -0.07276, 1.07602};
    const double gamma = 1.0 / 2.4;
    double p[4], c[3], f[3];
    for (int k = 0; k < 4; k++) p[k] = rgba[4 * i + k] * scale;
    for (int r = 0; r < 3; r++) c[r] = kIn[3 * r] * p[0] + kIn[3 * r + 1] * p[1] + kIn[3 * r + 2] * p[2] + 0.0 * p[3];
    for (int k = 0; k < 3; k++) {
        const double a = c[k] * (c[k] + 0.0245786) - 0.000090537;
        const double b = c[k] * (c[k] * 0.983729 + 0.4329510) + 0.238081;
        f[k] = a / b;
    }
    for (int r = 0; r < 3; r++) {
        double x = kOut[3 * r] * f[0] + kOut[3 * r + 1] * f[1] + kOut[3 * r + 2] * f[2] + 0.0 * 0.0;
        if (x < 0.0) x = 0.0;  // clamp01: NaN stays NaN
        if (x > 1.0) x = 1.0;
        const double v = x < 0.0031308 ? x * 12.92 : pow(x, gamma) * 1.055 - 0.055;
        const double q = v * 255.999;
        rgb[3 * i + r] = !(q > 0.0) ? uint8_t(0) : (q >= 255.0 ? uint8_t(255) : uint8_t(q));  // saturating `as u8`, NaN -> 0
    }
}

static int tonemap_launch(const double* d_rgba, uint64_t npix, double scale, uint8_t* d_rgb, hipStream_t stream) {
    if (npix == 0) return RT_OK;
    hipLaunchKernelGGL(k_tonemap_rgb8, dim3(uint32_t((npix + 255) / 256)), dim3(256), 0, stream, d_rgba, npix, scale, d_rgb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// The decision step of an adaptive accumulator (include/rt_mi355.h).
// ---------------------------------------------------------------------------------------------
// Pixel states of the decision step: a stopped pixel does not hold its neighbours, so it reads as quiet.
constexpr uint8_t AD_NOISY = 0, AD_QUIET = 1, AD_STOPPED = 2;

// se2 <= (threshold (mean + floor))^2 after k replicas; any NaN makes the comparison false.
RT_DEV bool ad_quiet(double m1, double m2, uint32_t k, double threshold, double floor_) {
#pragma clang fp contract(off)
    const double mean = m1 / double(k);
    double num = m2 - m1 * mean;
    if (num < 0.0) num = 0.0;
    const double se2 = num / (double(k) * double(k - 1u));
    const double lim = threshold * (mean + floor_);
    return se2 <= lim * lim;
}

// Decision, step 1: state[p] of every active pixel (every active pixel has n = k).
__global__ void __launch_bounds__(256) k_ad_quiet(const uint32_t* __restrict__ active, uint32_t n_active, const double* __restrict__ s1,
                                                  const double* __restrict__ s2, uint32_t k, double threshold, double floor_,
                                                  uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_active) return;
    const uint32_t p = active[i];
    state[p] = ad_quiet(s1[p], s2[p], k, threshold, floor_) ? AD_QUIET : AD_NOISY;
}

constexpr uint32_t AD_CHUNK = 2048;  // active-list entries per workgroup of the window and scatter kernels

// Decision, step 2: entry i stays (keep[i] = 1) unless its pixel is quiet and no pixel of its window is noisy; per workgroup
// the number of entries that stay.  Reads `state` only: the new states are written by k_ad_scatter.
__global__ void __launch_bounds__(256) k_ad_window(const uint32_t* __restrict__ active, uint32_t n_active, const uint8_t* __restrict__ state,
                                                   uint32_t width, uint32_t height, int radius, uint8_t* __restrict__ keep,
                                                   uint32_t* __restrict__ block_count) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint32_t begin = blockIdx.x * AD_CHUNK;
    const uint32_t end = min(n_active, begin + AD_CHUNK);
    uint32_t mine = 0;
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const uint32_t p = active[i];
        const int y = int(p / width), x = int(p - uint32_t(y) * width);
        bool stop = state[p] == AD_QUIET;
        for (int dy = -radius; stop && dy <= radius; dy++) {
            const int yy = y + dy;
            if (yy < 0 || yy >= int(height)) continue;
            for (int dx = -radius; dx <= radius; dx++) {
                const int xx = x + dx;
                if (xx < 0 || xx >= int(width)) continue;
                stop = stop && state[uint32_t(yy) * width + uint32_t(xx)] != AD_NOISY;
            }
        }
        keep[i] = stop ? 0 : 1;
        mine += stop ? 0u : 1u;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&total, mine);  // integer sum: the order does not matter
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// Decision, step 3: exclusive scan of the workgroup counts by one wave (in place), the total to *n_out.
__global__ void __launch_bounds__(64) k_ad_scan(uint32_t* __restrict__ block_count, uint32_t n_blocks, uint32_t* __restrict__ n_out) {
    const uint32_t lane = threadIdx.x;
    uint32_t base = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64) {
        const uint32_t b = b0 + lane;
        const uint32_t v = b < n_blocks ? block_count[b] : 0u;
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (int(lane) >= off) incl += o;
        }
        if (b < n_blocks) block_count[b] = base + incl - v;
        base += __shfl(incl, 63);
    }
    if (lane == 0) *n_out = base;
}

// Decision, step 4: order-preserving compaction of the active list (ballot prefix inside a wave, wave totals through LDS;
// no atomic decides a position); the pixels that leave the list become AD_STOPPED.
__global__ void __launch_bounds__(256) k_ad_scatter(const uint32_t* __restrict__ active, uint32_t n_active, const uint8_t* __restrict__ keep,
                                                    const uint32_t* __restrict__ block_offset, uint32_t* __restrict__ active_out,
                                                    uint8_t* __restrict__ state) {
    __shared__ uint32_t wave_total[4];
    const uint32_t begin = blockIdx.x * AD_CHUNK;
    const uint32_t end = min(n_active, begin + AD_CHUNK);
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t base = block_offset[blockIdx.x];
    for (uint32_t i0 = begin; i0 < end; i0 += blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        const bool in = i < end;
        const uint32_t p = in ? active[i] : 0u;
        const bool stay = in && keep[i] != 0;
        const unsigned long long m = __ballot(stay);
        if ((threadIdx.x & 63u) == 0) wave_total[wave] = uint32_t(__popcll(m));
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t c = wave_total[w];
            before += w < wave ? c : 0u;
            all += c;
        }
        if (stay) active_out[base + before + lane_prefix(m)] = p;
        else if (in) state[p] = AD_STOPPED;
        base += all;
        __syncthreads();
    }
}

// Rebuilds the list after a state load: pixel p is active iff n[p] == k.  Same scan, flags from the counts.
__global__ void __launch_bounds__(256) k_ad_flags_from_counts(const uint32_t* __restrict__ cnt, uint32_t npix, uint32_t k, uint32_t* __restrict__ identity,
                                                              uint8_t* __restrict__ keep, uint8_t* __restrict__ state, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint32_t begin = blockIdx.x * AD_CHUNK;
    const uint32_t end = min(npix, begin + AD_CHUNK);
    uint32_t mine = 0;
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const bool on = cnt[i] == k;
        identity[i] = i;
        keep[i] = on ? 1 : 0;
        state[i] = AD_NOISY;  // k_ad_scatter marks the others AD_STOPPED
        mine += on ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// estimate of an adaptive accumulator: sum[p] * (T / n[p]) (w stays 0; the factor is exactly 1 at n = T)
__global__ void __launch_bounds__(256) k_accum_estimate_adaptive(const double* __restrict__ sum, const uint32_t* __restrict__ cnt, uint64_t npix,
                                                                 double T, double* __restrict__ out) {
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const double scale = T / double(cnt[p]);
    for (int k = 0; k < 4; k++) out[4 * p + k] = sum[4 * p + k] * scale;
}

}  // namespace rt

struct RtAccum {
    RtScene* scene = nullptr;      // not owned: must outlive every call but rt_accum_destroy
    uint64_t generation = 0;       // the scene's generation at rt_accum_create: an accumulator does not outlive an rt_scene_update
    int device = 0;                // the scene's device (rt_accum_destroy does not touch the scene)
    RtCameraDesc camera{};
    RtRenderParams params{};       // as created (pipeline / collect_stats: the defaults of rt_accum_render)
    uint32_t owned = 0, T = 0, k = 0;
    uint64_t frame_digest = 0;
    rt::DevBuf<double> d_sum;      // sum_k, owned x width x 4 doubles: the accumulator's own buffer
    rt::DevBuf<double> d_est;      // estimate scratch (lazy)
    rt::DevBuf<uint8_t> d_rgb;     // preview scratch (lazy)
    rt::DevBuf<double> d_aov;      // first-hit AOVs of the denoised previews (lazy, owned x width x 8; not in the state blob)
    uint32_t aov_replicas = 0;     // replicas d_aov was rendered with (0: none yet)
    rt::DenoiseScratch dn;         // denoiser scratch (lazy)
    // adaptive mode (rt_accum_set_adaptive): moments, replica counts, the ascending list of active pixels (two buffers that
    // take turns at a compaction) and the decision step's scratch
    bool adaptive = false, touched = false;  // touched: a state has been loaded
    RtAdaptiveParams ap{};
    rt::DevBuf<double> d_s1, d_s2;
    rt::DevBuf<uint32_t> d_cnt, d_active[2];
    int cur = 0;
    uint32_t n_active = 0;
    rt::DevBuf<uint8_t> d_state, d_keep;
    rt::DevBuf<uint32_t> d_block, d_n_out;
    ~RtAccum() { (void)hipSetDevice(device); }  // before the members go: the owners do not switch devices
    size_t n_doubles() const { return size_t(owned) * camera.image_width * 4; }
    size_t npix() const { return size_t(owned) * camera.image_width; }
    // what rt_accum_state.h works on
    rt::AccumFields fields() const { return {params.precision, camera.image_width, owned, T, k, rt::scene_content_digest(scene), frame_digest, adaptive, ap}; }
    bool decision_point(uint32_t kk) const { return rt::decision_point(fields(), kk); }
};

// An accumulator belongs to the scene as it was when the accumulator was created.
static bool accum_is_stale(const RtAccum* acc) { return acc->generation != rt::scene_generation(acc->scene); }
static int accum_stale_error() { return rt::set_err(RT_E_INVALID, "the scene was updated after this accumulator was created"); }

extern "C" {

int rt_accum_create(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, RtAccum** out) {
    using namespace rt;
    if (!out) return set_err(RT_E_INVALID, "rt_accum_create: out is NULL");
    *out = nullptr;
    if (!scene || !camera || !params) return set_err(RT_E_INVALID, "rt_accum_create: NULL argument");
    if (int v = validate_render_args(camera, params)) return v;
    const uint32_t owned = owned_rows(camera->image_height, params);
    if (owned == 0) return set_err(RT_E_INVALID, "rt_accum_create: the row partition gives this part no rows");
    std::unique_ptr<RtAccum> a(new (std::nothrow) RtAccum);
    if (!a) return set_err(RT_E_NOMEM, "out of memory");
    a->scene = const_cast<RtScene*>(scene);
    a->generation = scene_generation(scene);
    a->device = scene_device(scene);
    a->camera = *camera;
    a->params = *params;
    a->owned = owned;
    a->T = params->thread_count;
    a->frame_digest = frame_digest(*camera, *params);
    HIP_TRY(hipSetDevice(a->device));
    if (int st = a->d_sum.reserve(a->n_doubles() * sizeof(double))) return st;
    HIP_TRY(hipMemset(a->d_sum, 0, a->n_doubles() * sizeof(double)));
    HIP_TRY(hipDeviceSynchronize());
    *out = a.release();
    return RT_OK;
}

void rt_accum_destroy(RtAccum* acc) { delete acc; }  // ~RtAccum sets the device

// Scan + scatter of the decision step: entries of `src` (n_src of them) with keep != 0 go, in order, to the other list, which
// becomes the active list; 4 bytes come back to the host.
static int adaptive_compact(RtAccum* a, const uint32_t* src, uint32_t n_src, hipStream_t st) {
    using namespace rt;
    const uint32_t n_blocks = (n_src + AD_CHUNK - 1) / AD_CHUNK;
    hipLaunchKernelGGL(k_ad_scan, dim3(1), dim3(64), 0, st, a->d_block.get(), n_blocks, a->d_n_out.get());
    hipLaunchKernelGGL(k_ad_scatter, dim3(n_blocks), dim3(256), 0, st, src, n_src, a->d_keep.get(), a->d_block.get(), a->d_active[a->cur ^ 1].get(), a->d_state.get());
    HIP_TRY(hipGetLastError());
    uint32_t n_new = 0;
    HIP_TRY(hipMemcpyAsync(&n_new, a->d_n_out, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_new > n_src) return set_err(RT_E_DEVICE, "adaptive compaction returned more pixels than it was given");
    a->cur ^= 1;
    a->n_active = n_new;
    return RT_OK;
}

// The decision at k = acc->k (a decision point): quiet flags, window rule, compaction of the active list.
static int adaptive_decide(RtAccum* a, hipStream_t st) {
    using namespace rt;
    if (a->n_active == 0) return RT_OK;
    const uint32_t n = a->n_active, n_blocks = (n + AD_CHUNK - 1) / AD_CHUNK;
    const uint32_t* list = a->d_active[a->cur];
    hipLaunchKernelGGL(k_ad_quiet, dim3((n + 255) / 256), dim3(256), 0, st, list, n, a->d_s1.get(), a->d_s2.get(), a->k, a->ap.threshold, a->ap.floor, a->d_state.get());
    hipLaunchKernelGGL(k_ad_window, dim3(n_blocks), dim3(256), 0, st, list, n, a->d_state.get(), a->camera.image_width, a->owned, int(a->ap.radius), a->d_keep.get(), a->d_block.get());
    return adaptive_compact(a, list, n, st);
}

// Active list from the counts (after a state load): n[p] == k, then the decision at k again if k is a decision point - it sees
// the sums it saw before the save, so it stops the same pixels.
static int adaptive_rebuild(RtAccum* a, hipStream_t st) {
    using namespace rt;
    const uint32_t n = uint32_t(a->npix()), n_blocks = (n + AD_CHUNK - 1) / AD_CHUNK;
    hipLaunchKernelGGL(k_ad_flags_from_counts, dim3(n_blocks), dim3(256), 0, st, a->d_cnt.get(), n, a->k, a->d_active[a->cur].get(), a->d_keep.get(), a->d_state.get(), a->d_block.get());
    if (int r = adaptive_compact(a, a->d_active[a->cur], n, st)) return r;
    if (a->decision_point(a->k)) return adaptive_decide(a, st);
    return RT_OK;
}

// rt_accum_render of an adaptive accumulator: segments that end at the decision points, a decision after each.
static int accum_render_adaptive(RtAccum* acc, uint32_t n_replicas, RtRenderParams p, void* stream) {
    using namespace rt;
    if (p.pipeline == RT_PIPELINE_MEGAKERNEL) return set_err(RT_E_UNSUPPORTED, "rt_accum_render: adaptive passes run the wavefront scheduler, RT_PIPELINE_MEGAKERNEL is not supported");
    if (p.collect_stats) return set_err(RT_E_UNSUPPORTED, "rt_accum_render: collect_stats is not supported on an adaptive accumulator");
    p.pipeline = RT_PIPELINE_WAVEFRONT;
    RtScene* s = acc->scene;
    HIP_TRY(hipSetDevice(acc->device));
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : scene_stream(s);
    uint32_t left = std::min(n_replicas, acc->T - acc->k);
    RtRenderStats total{};
    bool first = true;
    int32_t* const flag = scene_tail_flag(s);  // the call's end releases a waiting frame (rt_accum_render), not a segment's
    scene_set_tail_flag(s, nullptr);
    int r = RT_OK;
    while (left > 0 && acc->n_active > 0) {
        const uint32_t next = next_segment_end(acc->fields());
        const uint32_t m = std::min(left, next - acc->k);
        AdaptivePass ad;
        ad.active = acc->d_active[acc->cur];
        ad.n_active = acc->n_active;
        ad.sparse = acc->n_active < acc->npix();
        ad.s1 = acc->d_s1; ad.s2 = acc->d_s2; ad.cnt = acc->d_cnt;
        r = render_replicas(s, &acc->camera, &p, acc->k, m, acc->d_sum, st, &ad);
        if (r != RT_OK) break;
        stats_add(total, scene_stats(s), first);
        first = false;
        acc->k += m;
        left -= m;
        if (acc->decision_point(acc->k) && (r = adaptive_decide(acc, st)) != RT_OK) break;
    }
    scene_set_tail_flag(s, flag);
    if (!first) scene_set_stats(s, total);
    else if (r == RT_OK) {  // nothing rendered
        RtRenderStats none{};
        none.pipeline_used = RT_PIPELINE_WAVEFRONT;
        scene_set_stats(s, none);
    }
    return r;
}

static int accum_render_impl(RtAccum* acc, uint32_t n_replicas, const RtRenderParams* params_or_null, void* stream) {
    using namespace rt;
    if (!acc) return set_err(RT_E_INVALID, "rt_accum_render: NULL accumulator");
    if (accum_is_stale(acc)) return accum_stale_error();
    RtRenderParams p = acc->params;
    if (params_or_null) {
        const RtRenderParams a = frame_fields(acc->params), b = frame_fields(*params_or_null);
        if (std::memcmp(&a, &b, sizeof a) != 0)
            return set_err(RT_E_INVALID, "rt_accum_render: params differ from the accumulator's in more than pipeline / collect_stats");
        p.pipeline = params_or_null->pipeline;
        p.collect_stats = params_or_null->collect_stats;
    }
    if (acc->adaptive) return accum_render_adaptive(acc, n_replicas, p, stream);
    const uint32_t n = std::min(n_replicas, acc->T - acc->k);
    if (n == 0) return RT_OK;
    const int r = render_replicas(acc->scene, &acc->camera, &p, acc->k, n, acc->d_sum, stream);
    if (r == RT_OK) acc->k += n;
    return r;
}

int rt_accum_render(RtAccum* acc, uint32_t n_replicas, const RtRenderParams* params_or_null, void* stream) {
    const int r = accum_render_impl(acc, n_replicas, params_or_null, stream);
    if (acc) rt::scene_release_tail(acc->scene);  // as rt_render_device does
    return r;
}

uint32_t rt_accum_replicas_done(const RtAccum* acc) { return acc ? acc->k : 0; }

// The estimate of sum_k into the device buffer d_out (stream: NULL = the scene's stream; returns after it is complete).
static int accum_estimate_to(const RtAccum* acc, double* d_out, hipStream_t stream) {
    using namespace rt;
    const size_t n = acc->n_doubles();
    if (acc->adaptive) {
        hipLaunchKernelGGL(k_accum_estimate_adaptive, dim3(uint32_t((n / 4 + 255) / 256)), dim3(256), 0, stream, acc->d_sum.get(), acc->d_cnt.get(), uint64_t(n / 4),
                           double(acc->T), d_out);
        HIP_TRY(hipGetLastError());
    } else if (acc->k == acc->T) {  // factor 1: the estimate is the frame, bit for bit
        HIP_TRY(hipMemcpyAsync(d_out, acc->d_sum, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    } else {
        hipLaunchKernelGGL(k_accum_estimate, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, stream, acc->d_sum.get(), uint64_t(n),
                           double(acc->T) / double(acc->k), d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

static int accum_check_estimate(const RtAccum* acc, const void* out, const char* who) {
    if (!acc || !out) return rt::set_err(RT_E_INVALID, std::string(who) + ": NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    if (acc->k == 0) return rt::set_err(RT_E_INVALID, std::string(who) + ": no replica rendered yet (k = 0)");
    return RT_OK;
}

int rt_accum_estimate_device(const RtAccum* acc, double* d_rgba_out, void* stream) {
    using namespace rt;
    if (int v = accum_check_estimate(acc, d_rgba_out, "rt_accum_estimate_device")) return v;
    HIP_TRY(hipSetDevice(acc->device));
    return accum_estimate_to(acc, d_rgba_out, stream ? static_cast<hipStream_t>(stream) : scene_stream(acc->scene));
}

static int accum_scratch(RtAccum* a) {
    using namespace rt;
    if (int st = a->d_est.reserve(a->n_doubles() * sizeof(double))) return st;
    return a->d_rgb.reserve(a->n_doubles() / 4 * 3);
}

int rt_accum_estimate(const RtAccum* acc, double* rgba_out) {
    using namespace rt;
    if (int v = accum_check_estimate(acc, rgba_out, "rt_accum_estimate")) return v;
    HIP_TRY(hipSetDevice(acc->device));
    RtAccum* a = const_cast<RtAccum*>(acc);  // scratch buffers only
    if (int st = accum_scratch(a)) return st;
    if (int st = accum_estimate_to(a, a->d_est, scene_stream(a->scene))) return st;
    HIP_TRY(hipMemcpy(rgba_out, a->d_est, a->n_doubles() * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_accum_preview_rgb8(const RtAccum* acc, uint8_t* rgb_out) {
    using namespace rt;
    if (int v = accum_check_estimate(acc, rgb_out, "rt_accum_preview_rgb8")) return v;
    HIP_TRY(hipSetDevice(acc->device));
    RtAccum* a = const_cast<RtAccum*>(acc);
    if (int st = accum_scratch(a)) return st;
    const double scale = a->k == a->T ? 1.0 : double(a->T) / double(a->k);  // the estimate, formed inside the kernel
    if (a->adaptive) {  // per-pixel factors: the estimate first
        if (int st = accum_estimate_to(a, a->d_est, scene_stream(a->scene))) return st;
        if (int st = tonemap_launch(a->d_est, a->n_doubles() / 4, 1.0, a->d_rgb, scene_stream(a->scene))) return st;
    } else if (int st = tonemap_launch(a->d_sum, a->n_doubles() / 4, scale, a->d_rgb, scene_stream(a->scene))) {
        return st;
    }
    HIP_TRY(hipMemcpy(rgb_out, a->d_rgb, a->n_doubles() / 4 * 3, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_tonemap_rgb8_device(int device, const double* d_rgba, uint32_t width, uint32_t height, uint8_t* d_rgb, void* stream) {
    using namespace rt;
    if (!d_rgba || !d_rgb) return set_err(RT_E_INVALID, "rt_tonemap_rgb8_device: NULL argument");
    HIP_TRY(hipSetDevice(device));
    return tonemap_launch(d_rgba, uint64_t(width) * height, 1.0, d_rgb, static_cast<hipStream_t>(stream));
}

size_t rt_accum_state_size(const RtAccum* acc) {
    if (!acc) return 0;
    return rt::accum_state_size(acc->adaptive, acc->owned, acc->camera.image_width);
}

int rt_accum_save_state(const RtAccum* acc, void* buf, size_t size) {
    using namespace rt;
    if (!acc || !buf) return set_err(RT_E_INVALID, "rt_accum_save_state: NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    if (size < rt_accum_state_size(acc)) return set_err(RT_E_INVALID, "rt_accum_save_state: buffer smaller than rt_accum_state_size");
    const AccumHeader h = accum_header(acc->fields());
    HIP_TRY(hipSetDevice(acc->device));
    char* body = static_cast<char*>(buf) + sizeof h;
    if (acc->adaptive) {
        const AdaptiveBlobParams bp = blob_params(acc->ap);
        std::memcpy(body, &bp, sizeof bp);
        body += sizeof bp;
    }
    HIP_TRY(hipMemcpy(body, acc->d_sum, acc->n_doubles() * sizeof(double), hipMemcpyDeviceToHost));
    if (acc->adaptive) {
        const size_t np = acc->npix();
        body += np * 32;
        HIP_TRY(hipMemcpy(body, acc->d_s1, np * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(body + np * 8, acc->d_s2, np * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(body + np * 16, acc->d_cnt, np * 4, hipMemcpyDeviceToHost));
    }
    std::memcpy(buf, &h, sizeof h);
    return RT_OK;
}

int rt_accum_load_state(RtAccum* acc, const void* buf, size_t size) {
    using namespace rt;
    if (!acc || !buf) return set_err(RT_E_INVALID, "rt_accum_load_state: NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    AccumHeader h;
    if (int v = accum_check_state(acc->fields(), buf, size, &h)) return v;
    const char* body = static_cast<const char*>(buf) + sizeof h + (acc->adaptive ? sizeof(AdaptiveBlobParams) : 0);
    const size_t np = acc->npix();
    HIP_TRY(hipSetDevice(acc->device));
    HIP_TRY(hipMemcpy(acc->d_sum, body, acc->n_doubles() * sizeof(double), hipMemcpyHostToDevice));
    if (acc->adaptive) {
        HIP_TRY(hipMemcpy(acc->d_s1, body + np * 32, np * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(acc->d_s2, body + np * 40, np * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(acc->d_cnt, body + np * 48, np * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipDeviceSynchronize());  // the render kernels run on a non-blocking stream, not ordered against this copy
    acc->k = h.replicas_done;
    acc->touched = true;
    if (acc->adaptive) return adaptive_rebuild(acc, scene_stream(acc->scene));
    return RT_OK;
}

// ---- The denoised previews (the filter: rt_aov.hip) --------------------------------------------------------------
// The denoised estimate of `a` into a->d_est (scene's stream, complete on return).  Renders the AOVs on first use.
static int accum_denoise(RtAccum* a, const RtDenoiseParams* dp, const char* who) {
    using namespace rt;
    RtDenoiseParams p;
    if (int v = denoise_params(dp, &p, who)) return v;
    if (a->params.band_rows != 0 && a->params.n_parts > 1)
        return set_err(RT_E_INVALID, std::string(who) + ": the accumulator has a row partition (the filter needs contiguous rows)");
    if (p.aov_replicas == 0 || p.aov_replicas > a->T) return set_err(RT_E_INVALID, std::string(who) + ": aov_replicas must be in 1 .. thread_count");
    HIP_TRY(hipSetDevice(a->device));
    if (int st = accum_scratch(a)) return st;
    const uint32_t w = a->camera.image_width;
    if (a->aov_replicas != p.aov_replicas) {
        if (int st = a->d_aov.reserve(size_t(a->owned) * w * kAovChannels * sizeof(double))) return st;
        a->aov_replicas = 0;
        if (int st = render_aov_replicas(a->scene, &a->camera, &a->params, p.aov_replicas, a->d_aov, nullptr)) return st;
        a->aov_replicas = p.aov_replicas;
    }
    if (int st = accum_estimate_to(a, a->d_est, scene_stream(a->scene))) return st;
    return denoise_run(a->d_est, a->d_aov, w, a->owned, p, a->d_est, &a->dn, scene_stream(a->scene));
}

int rt_accum_estimate_denoised(const RtAccum* acc, const RtDenoiseParams* dp, double* rgba_out) {
    using namespace rt;
    if (int v = accum_check_estimate(acc, rgba_out, "rt_accum_estimate_denoised")) return v;
    RtAccum* a = const_cast<RtAccum*>(acc);  // scratch buffers and the AOV cache only
    if (int st = accum_denoise(a, dp, "rt_accum_estimate_denoised")) return st;
    HIP_TRY(hipMemcpy(rgba_out, a->d_est, a->n_doubles() * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_accum_preview_denoised_rgb8(const RtAccum* acc, const RtDenoiseParams* dp, uint8_t* rgb_out) {
    using namespace rt;
    if (int v = accum_check_estimate(acc, rgb_out, "rt_accum_preview_denoised_rgb8")) return v;
    RtAccum* a = const_cast<RtAccum*>(acc);
    if (int st = accum_denoise(a, dp, "rt_accum_preview_denoised_rgb8")) return st;
    if (int st = tonemap_launch(a->d_est, a->n_doubles() / 4, 1.0, a->d_rgb, scene_stream(a->scene))) return st;
    HIP_TRY(hipMemcpy(rgb_out, a->d_rgb, a->n_doubles() / 4 * 3, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- Adaptive mode ------------------------------------------------------------------------
int rt_adaptive_default_params(RtAdaptiveParams* out) {
    if (!out) return rt::set_err(RT_E_INVALID, "rt_adaptive_default_params: NULL argument");
    *out = RtAdaptiveParams{};
    out->floor = 0.01;  // the values of the oracle experiment; the threshold has no default
    out->min_replicas = 4;
    out->check_interval = 2;
    out->radius = 1;
    return RT_OK;
}

int rt_accum_set_adaptive(RtAccum* acc, const RtAdaptiveParams* ap) {
    using namespace rt;
    if (!acc || !ap) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    if (acc->adaptive) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: the accumulator is adaptive already");
    if (acc->k != 0 || acc->touched) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: only before the first replica and before a state is loaded");
    if (int v = adaptive_params_check(ap, acc->params, acc->npix())) return v;
    HIP_TRY(hipSetDevice(acc->device));
    const size_t np = acc->npix(), n_blocks = (np + AD_CHUNK - 1) / AD_CHUNK;
    // local owners first: a failure half way leaves the accumulator as it was
    DevBuf<double> s1, s2;
    DevBuf<uint32_t> cnt, a0, a1, block, n_out;
    DevBuf<uint8_t> state, keep;
    auto zeroed = [](auto& buf, size_t bytes) -> int {
        if (int st = buf.reserve(bytes)) return st;
        HIP_TRY(hipMemset(buf, 0, bytes));
        return RT_OK;
    };
    int st;
    if ((st = zeroed(s1, np * 8)) || (st = zeroed(s2, np * 8)) || (st = zeroed(cnt, np * 4)) || (st = zeroed(a0, np * 4)) || (st = zeroed(a1, np * 4)) ||
        (st = zeroed(state, np)) || (st = zeroed(keep, np)) || (st = zeroed(block, n_blocks * 4)) || (st = zeroed(n_out, 4))) return st;
    {  // every pixel is active, in ascending order
        std::vector<uint32_t> identity(np);
        for (size_t i = 0; i < np; i++) identity[i] = uint32_t(i);
        HIP_TRY(hipMemcpy(a0, identity.data(), np * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipDeviceSynchronize());
    acc->d_s1 = std::move(s1); acc->d_s2 = std::move(s2); acc->d_cnt = std::move(cnt);
    acc->d_active[0] = std::move(a0); acc->d_active[1] = std::move(a1);
    acc->d_state = std::move(state); acc->d_keep = std::move(keep);
    acc->d_block = std::move(block); acc->d_n_out = std::move(n_out);
    acc->cur = 0;
    acc->n_active = uint32_t(np);  // all pixels: the dense kernels run until the first pixel stops (the list is not read)
    acc->ap = *ap;
    acc->adaptive = true;
    return RT_OK;
}

uint32_t rt_accum_active_pixels(const RtAccum* acc) {
    if (!acc) return 0;
    if (acc->k >= acc->T) return 0;
    return acc->adaptive ? acc->n_active : uint32_t(acc->npix());
}

int rt_accum_finished(const RtAccum* acc) {
    if (!acc) return 0;
    return (acc->k >= acc->T || (acc->adaptive && acc->n_active == 0)) ? 1 : 0;
}

int rt_accum_sample_counts(const RtAccum* acc, uint32_t* counts_out) {
    using namespace rt;
    if (!acc || !counts_out) return set_err(RT_E_INVALID, "rt_accum_sample_counts: NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    if (!acc->adaptive) {
        std::fill(counts_out, counts_out + acc->npix(), acc->k);
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(acc->device));
    HIP_TRY(hipMemcpy(counts_out, acc->d_cnt, acc->npix() * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_accum_noise(const RtAccum* acc, double* noise_out) {
    using namespace rt;
    if (!acc || !noise_out) return set_err(RT_E_INVALID, "rt_accum_noise: NULL argument");
    if (accum_is_stale(acc)) return accum_stale_error();
    if (!acc->adaptive) return set_err(RT_E_INVALID, "rt_accum_noise: the accumulator keeps no moments (rt_accum_set_adaptive)");
    HIP_TRY(hipSetDevice(acc->device));
    const size_t np = acc->npix();
    std::vector<double> s1(np), s2(np);
    std::vector<uint32_t> cnt(np);
    HIP_TRY(hipMemcpy(s1.data(), acc->d_s1, np * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s2.data(), acc->d_s2, np * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cnt.data(), acc->d_cnt, np * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < np; i++) noise_out[i] = accum_noise(s1[i], s2[i], cnt[i], acc->ap.floor);  // a few flops per pixel on 20 bytes that cross the bus anyway
    return RT_OK;
}

}  // extern "C"
