// rt_accum_state.h — the host arithmetic of the progressive accumulator (rt_accum.hip), plain C++ without HIP: the state
// blob's layout and every check of a blob that needs no device, the frame digest, the parameter checks of
// rt_accum_set_adaptive, the segment schedule of an adaptive render and the noise formula.  rt_accum.hip calls these and
// keeps no copy of any; tools/accum_state_check.cpp runs them under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rt_mi355.h"
#include "rt_error.h"
#include "rt_tables.h"

namespace rt {

// The camera and every params field that changes the frame (all but pipeline and collect_stats).
inline RtRenderParams frame_fields(const RtRenderParams& p) {
    RtRenderParams q = p;
    q.pipeline = 0;
    q.collect_stats = 0;
    return q;
}
inline uint64_t frame_digest(const RtCameraDesc& c, const RtRenderParams& p) {
    Digest g;
    g.val(c.image_width); g.val(c.image_height); g.val(c.position); g.val(c.first_pixel); g.val(c.pixel_delta_u);
    g.val(c.pixel_delta_v); g.val(c.basis_u); g.val(c.basis_v); g.val(c.has_aperture); g.val(c.aperture_radius);
    const RtRenderParams q = frame_fields(p);
    g.val(q.sqrt_spt); g.val(q.thread_count); g.val(q.max_depth); g.val(q.has_background); g.val(q.light_bias);
    g.val(q.background); g.val(q.seed); g.val(q.band_rows); g.val(q.n_parts); g.val(q.part); g.val(q.precision);
    return g.value();
}

// State blob: this header (little-endian), then owned_rows * width * 4 doubles of sum_k
struct AccumHeader {
    char magic[8];
    uint32_t version, precision, width, owned_rows, thread_count, replicas_done;
    uint64_t scene_digest, frame_digest;
};
static_assert(sizeof(AccumHeader) == 48, "state header layout");
static const char kAccumMagic[8] = {'R', 'T', 'A', 'C', 'C', 'U', 'M', '\0'};
static const uint32_t kAccumVersion = 1;
static const uint32_t kAccumVersionAdaptive = 2;  // header, AdaptiveBlobParams, sum, s1, s2, n
struct AdaptiveBlobParams {
    double threshold, floor;
    uint32_t min_replicas, check_interval, radius, zero;
};
static_assert(sizeof(AdaptiveBlobParams) == 32, "state parameter block layout");
inline AdaptiveBlobParams blob_params(const RtAdaptiveParams& p) { return AdaptiveBlobParams{p.threshold, p.floor, p.min_replicas, p.check_interval, p.radius, 0u}; }

// The accumulator's plain fields: what a blob is written from and checked against, and what the schedule reads.
struct AccumFields {
    uint32_t precision = 0, width = 0, owned = 0, T = 0, k = 0;
    uint64_t scene_digest = 0, frame_digest = 0;
    bool adaptive = false;
    RtAdaptiveParams ap{};
    size_t npix() const { return size_t(owned) * width; }
};

inline size_t accum_state_size(bool adaptive, uint32_t owned, uint32_t width) {
    const size_t np = size_t(owned) * width;
    if (adaptive) return sizeof(AccumHeader) + sizeof(AdaptiveBlobParams) + np * (4 * 8 + 8 + 8 + 4);
    return sizeof(AccumHeader) + np * 4 * sizeof(double);
}

inline AccumHeader accum_header(const AccumFields& a) {
    AccumHeader h{};
    std::memcpy(h.magic, kAccumMagic, 8);
    h.version = a.adaptive ? kAccumVersionAdaptive : kAccumVersion;
    h.precision = a.precision;
    h.width = a.width;
    h.owned_rows = a.owned;
    h.thread_count = a.T;
    h.replicas_done = a.k;
    h.scene_digest = a.scene_digest;
    h.frame_digest = a.frame_digest;
    return h;
}

// D = { kk : min_replicas <= kk < T, (kk - min_replicas) mod check_interval = 0 } of an adaptive accumulator
inline bool decision_point(const AccumFields& a, uint32_t kk) {
    return a.adaptive && kk >= a.ap.min_replicas && kk < a.T && (kk - a.ap.min_replicas) % a.ap.check_interval == 0;
}

// Where the segment that starts at a.k ends: the next decision point, or T.
inline uint32_t next_segment_end(const AccumFields& a) {
    uint32_t next = a.T;
    if (a.k < a.ap.min_replicas) next = std::min(a.T, a.ap.min_replicas);
    else if (a.k < a.T) next = uint32_t(std::min<uint64_t>(a.T, uint64_t(a.k) + a.ap.check_interval - (a.k - a.ap.min_replicas) % a.ap.check_interval));
    return next;
}

// Every check of rt_accum_load_state that needs no device, on the `size` bytes at `buf` (nothing beyond them is read);
// *h is the blob's header once the blob is long enough to have one.
inline int accum_check_state(const AccumFields& a, const void* buf, size_t size, AccumHeader* h_out) {
    AccumHeader& h = *h_out;
    if (size < sizeof h) return set_err(RT_E_INVALID, "rt_accum_load_state: state truncated (shorter than its header)");
    std::memcpy(&h, buf, sizeof h);
    auto bad = [](const std::string& what) { return set_err(RT_E_INVALID, "rt_accum_load_state: " + what); };
    if (std::memcmp(h.magic, kAccumMagic, 8) != 0) return bad("not an accumulator state (wrong magic)");
    const uint32_t want_version = a.adaptive ? kAccumVersionAdaptive : kAccumVersion;
    if (h.version != want_version)
        return bad("state format version " + std::to_string(h.version) + ", expected " + std::to_string(want_version) +
                   (a.adaptive ? " (an adaptive accumulator)" : " (a plain accumulator)"));
    if (h.precision != a.precision) return bad("precision mismatch (state " + std::to_string(h.precision) + ", accumulator " + std::to_string(a.precision) + ")");
    if (h.width != a.width || h.owned_rows != a.owned)
        return bad("image size mismatch (state " + std::to_string(h.width) + " x " + std::to_string(h.owned_rows) + " rows, accumulator " +
                   std::to_string(a.width) + " x " + std::to_string(a.owned) + ")");
    if (h.thread_count != a.T) return bad("thread_count mismatch (state " + std::to_string(h.thread_count) + ", accumulator " + std::to_string(a.T) + ")");
    if (h.replicas_done > h.thread_count) return bad("state claims more replicas than thread_count");
    if (h.scene_digest != a.scene_digest) return bad("scene mismatch (the state was rendered from another scene description)");
    if (h.frame_digest != a.frame_digest) return bad("camera / render parameter mismatch (seed, camera, depth, light bias, background or row partition)");
    const size_t want_size = accum_state_size(a.adaptive, a.owned, a.width);
    if (size != want_size) return bad("state truncated or oversized (" + std::to_string(size) + " bytes, expected " + std::to_string(want_size) + ")");
    if (a.adaptive) {
        const char* body = static_cast<const char*>(buf) + sizeof h;
        const size_t np = a.npix();
        const AdaptiveBlobParams mine = blob_params(a.ap);
        if (std::memcmp(body, &mine, sizeof mine) != 0) return bad("adaptive parameter mismatch (threshold, floor, min_replicas, check_interval or radius)");
        body += sizeof mine;
        const char* cnt = body + np * 48;
        for (size_t i = 0; i < np; i++) {
            uint32_t c;
            std::memcpy(&c, cnt + 4 * i, 4);
            if (c > h.replicas_done || (c < h.replicas_done && !decision_point(a, c))) return bad("a pixel's replica count is neither the state's nor a decision point");
        }
    }
    return RT_OK;
}

// The parameter checks of rt_accum_set_adaptive on an accumulator of `npix` pixels created with `params`.
inline int adaptive_params_check(const RtAdaptiveParams* ap, const RtRenderParams& params, uint64_t npix) {
    if (!(ap->threshold > 0.0) || !std::isfinite(ap->threshold)) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: threshold must be positive and finite (it has no default)");
    if (!(ap->floor > 0.0) || !std::isfinite(ap->floor)) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: floor must be positive and finite");
    if (ap->min_replicas < 2) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: min_replicas must be at least 2 (a variance needs two replicas)");
    if (ap->check_interval < 1) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: check_interval must be at least 1");
    if (ap->radius > 4) return set_err(RT_E_INVALID, "rt_accum_set_adaptive: radius must be in 0 .. 4");
    if (params.band_rows != 0 && params.n_parts > 1)
        return set_err(RT_E_INVALID, "rt_accum_set_adaptive: the accumulator has a row partition (the window needs contiguous rows)");
    if (params.max_depth == 0) return set_err(RT_E_UNSUPPORTED, "rt_accum_set_adaptive: max_depth = 0 (adaptive passes run the wavefront scheduler)");
    if (npix >= (1ull << 31)) return set_err(RT_E_UNSUPPORTED, "rt_accum_set_adaptive: more than 2^31 pixels");
    return RT_OK;
}

// rt_accum_noise of one pixel: the standard error of the mean of its k luminances over (mean + floor), 0 below two replicas.
inline double accum_noise(double s1, double s2, uint32_t k, double floor) {
    if (k < 2) return 0.0;
    const double mean = s1 / double(k);
    double num = s2 - s1 * mean;
    if (num < 0.0) num = 0.0;
    return std::sqrt(num / (double(k) * double(k - 1))) / (mean + floor);
}

}  // namespace rt
