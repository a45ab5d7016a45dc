// accum_state_check.cpp — the host arithmetic of the progressive accumulator (csrc/rt_accum_state.h) as a stand-alone program,
// for sanitizer runs (no HIP include path: the header needs none, and nothing else is linked):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o accum_state_check
//       tools/accum_state_check.cpp && ./accum_state_check
// A 3 x 2 frame with T = 6 (adaptive: min_replicas 2, check_interval 2, radius 1).  State blobs in heap buffers of exactly their
// length: the round trip, every wrong length, every single corrupted field and pairs of them (the earlier check's message
// wins), the per-pixel replica-count rule; the segment schedule against brute force over decision_point; the refusals of
// rt_accum_set_adaptive's parameter checks; the noise formula.  Ends with a non-zero status on a failed check of its own.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include "../rust_raytracer_amd/csrc/rt_accum_state.h"

using namespace rt;

#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } } while (0)

static AccumFields fields(bool adaptive, uint32_t k) {
    AccumFields a;
    a.precision = RT_PRECISION_F64;
    a.width = 3; a.owned = 2; a.T = 6; a.k = k;
    a.scene_digest = 0x1122334455667788ull;
    a.frame_digest = 0x99AABBCCDDEEFF00ull;
    a.adaptive = adaptive;
    a.ap.threshold = 0.05; a.ap.floor = 0.01;
    a.ap.min_replicas = 2; a.ap.check_interval = 2; a.ap.radius = 1;
    return a;
}

// A heap buffer of exactly n bytes (n = 0: an allocation of which no byte may be read).
struct Bytes {
    size_t n;
    std::unique_ptr<char[]> p;
    explicit Bytes(size_t n_) : n(n_), p(new char[n_]()) {}
    Bytes(const Bytes& from, size_t n_) : Bytes(n_) { std::memcpy(p.get(), from.p.get(), std::min(n_, from.n)); }  // prefix, or zero-extended
    template <typename T> void put(size_t at, const T& v) { std::memcpy(p.get() + at, &v, sizeof v); }
};

// Where pixel i's replica count is in an adaptive blob: header, parameter block, sum (32 B a pixel), s1, s2, then the counts.
static size_t count_at(const AccumFields& a, size_t i) { return sizeof(AccumHeader) + sizeof(AdaptiveBlobParams) + a.npix() * 48 + 4 * i; }

// The blob rt_accum_save_state writes for `a`: sums of zero, every pixel with a.k replicas.
static Bytes blob_of(const AccumFields& a) {
    Bytes b(accum_state_size(a.adaptive, a.owned, a.width));
    b.put(0, accum_header(a));
    if (a.adaptive) {
        b.put(sizeof(AccumHeader), blob_params(a.ap));
        for (size_t i = 0; i < a.npix(); i++) b.put(count_at(a, i), a.k);
    }
    return b;
}

static int load(const AccumFields& a, const Bytes& b) {
    AccumHeader h;
    g_err.clear();
    return accum_check_state(a, b.p.get(), b.n, &h);
}
// refused with RT_E_INVALID and a message that contains `with`; prints the message
static bool refused(const AccumFields& a, const Bytes& b, const char* with) {
    const int st = load(a, b);
    std::printf("  %s\n", g_err.c_str());
    return st == RT_E_INVALID && g_err.find(with) != std::string::npos;
}

static int check_lengths(const AccumFields& a) {
    const Bytes full = blob_of(a);
    size_t n_refused = 0;
    for (size_t len = 0; len <= full.n + 1; len++) {
        if (len == full.n) continue;
        const Bytes b(full, len);
        CHECK(load(a, b) == RT_E_INVALID && g_err.find("truncated") != std::string::npos);
        CHECK((len < sizeof(AccumHeader)) == (g_err.find("shorter than its header") != std::string::npos));
        n_refused++;
    }
    std::printf("lengths (%s): %zu of %zu refused as truncated, %zu accepted\n", a.adaptive ? "adaptive" : "plain", n_refused, full.n + 1, full.n);
    return 0;
}

// One header field of a valid blob replaced by `v`.
template <typename T>
static Bytes with_field(const Bytes& full, size_t at, T v) {
    Bytes b(full, full.n);
    b.put(at, v);
    return b;
}

static int check_corruptions() {
    const AccumFields ad = fields(true, 4), plain = fields(false, 4);
    const Bytes full = blob_of(ad), full_plain = blob_of(plain);
    CHECK(full.n == 48 + 32 + 6 * 52 && full_plain.n == 48 + 6 * 32);
    CHECK(load(ad, full) == RT_OK && load(plain, full_plain) == RT_OK);
    std::printf("round trip: plain %zu bytes, adaptive %zu bytes\n", full_plain.n, full.n);
#define AT(field) offsetof(AccumHeader, field)
    std::printf("single corruptions:\n");
    CHECK(refused(ad, with_field(full, AT(magic), 'X'), "wrong magic"));
    CHECK(refused(ad, with_field(full, AT(version), kAccumVersion), "state format version"));              // a plain state into an adaptive accumulator
    CHECK(refused(plain, with_field(full_plain, AT(version), kAccumVersionAdaptive), "state format version"));  // and the other way round
    CHECK(refused(ad, with_field(full, AT(precision), uint32_t(RT_PRECISION_F32)), "precision mismatch"));
    CHECK(refused(ad, with_field(full, AT(width), 4u), "image size mismatch"));
    CHECK(refused(ad, with_field(full, AT(owned_rows), 1u), "image size mismatch"));
    CHECK(refused(ad, with_field(full, AT(thread_count), 7u), "thread_count mismatch"));
    CHECK(refused(ad, with_field(full, AT(replicas_done), 7u), "more replicas than thread_count"));
    CHECK(refused(ad, with_field(full, AT(scene_digest), uint64_t(1)), "scene mismatch"));
    CHECK(refused(ad, with_field(full, AT(frame_digest), uint64_t(1)), "camera / render parameter mismatch"));
    CHECK(refused(ad, with_field(full, sizeof(AccumHeader) + offsetof(AdaptiveBlobParams, radius), 2u), "adaptive parameter mismatch"));
    CHECK(refused(ad, with_field(full, sizeof(AccumHeader) + offsetof(AdaptiveBlobParams, zero), 1u), "adaptive parameter mismatch"));
    std::printf("pairs, the earlier check's message:\n");
    {
        Bytes b = with_field(full, AT(magic), 'X');
        b.put(AT(version), 9u);
        CHECK(refused(ad, b, "wrong magic"));
        b = with_field(full, AT(precision), uint32_t(RT_PRECISION_F32));
        b.put(AT(thread_count), 7u);
        CHECK(refused(ad, b, "precision mismatch"));
        b = with_field(full, AT(scene_digest), uint64_t(1));
        b.put(AT(frame_digest), uint64_t(1));
        CHECK(refused(ad, b, "scene mismatch"));
        b = with_field(full, AT(width), 4u);
        b.put(sizeof(AccumHeader) + offsetof(AdaptiveBlobParams, radius), 2u);
        CHECK(refused(ad, b, "image size mismatch"));
        const Bytes shorter(with_field(full, AT(frame_digest), uint64_t(1)), full.n - 1);  // the size check comes after the digests
        CHECK(refused(ad, shorter, "camera / render parameter mismatch"));
        b = with_field(full, sizeof(AccumHeader) + offsetof(AdaptiveBlobParams, radius), 2u);
        b.put(count_at(ad, 0), 5u);
        CHECK(refused(ad, b, "adaptive parameter mismatch"));
    }
#undef AT
    return 0;
}

static int check_counts() {
    const AccumFields a = fields(true, 5);
    const Bytes full = blob_of(a);
    CHECK(load(a, full) == RT_OK);
    std::printf("replica counts at k = 5:\n");
    CHECK(refused(a, with_field(full, count_at(a, 5), 6u), "neither the state's nor a decision point"));  // more than the state's
    CHECK(refused(a, with_field(full, count_at(a, 2), 3u), "neither the state's nor a decision point"));  // 3 is no decision point
    CHECK(load(a, with_field(full, count_at(a, 0), 4u)) == RT_OK);
    CHECK(load(a, with_field(full, count_at(a, 3), 2u)) == RT_OK);
    std::printf("  4 and 2 accepted\n");
    return 0;
}

static int check_schedule() {
    size_t n = 0;
    for (uint32_t T = 1; T <= 12; T++)
        for (uint32_t mn = 2; mn <= 6; mn++)
            for (uint32_t iv = 1; iv <= 4; iv++)
                for (uint32_t k = 0; k < T; k++) {
                    AccumFields a = fields(true, k);
                    a.T = T; a.ap.min_replicas = mn; a.ap.check_interval = iv;
                    uint32_t want = T;
                    for (uint32_t kk = k + 1; kk < T; kk++)
                        if (decision_point(a, kk)) { want = kk; break; }
                    CHECK(next_segment_end(a) == want);
                    n++;
                }
    std::printf("segment schedule: %zu cases equal brute force\n", n);
    const uint32_t shown[3][3] = {{6, 2, 2}, {12, 3, 4}, {4, 4, 1}};
    for (const auto& c : shown) {
        AccumFields a = fields(true, 0);
        a.T = c[0]; a.ap.min_replicas = c[1]; a.ap.check_interval = c[2];
        std::printf("decision points T=%u min_replicas=%u check_interval=%u:", c[0], c[1], c[2]);
        for (uint32_t kk = 0; kk <= a.T; kk++)
            if (decision_point(a, kk)) std::printf(" %u", kk);
        std::printf("\n");
        a.adaptive = false;  // a plain accumulator has none
        for (uint32_t kk = 0; kk <= a.T; kk++) CHECK(!decision_point(a, kk));
    }
    return 0;
}

static int check_adaptive_params() {
    const AccumFields a = fields(true, 0);
    RtRenderParams params{};
    params.max_depth = 8;
    CHECK(adaptive_params_check(&a.ap, params, a.npix()) == RT_OK);
    std::printf("rt_accum_set_adaptive refusals:\n");
    auto refuses = [&](const RtAdaptiveParams& ap, const RtRenderParams& p, uint64_t npix, int status, const char* with) {
        g_err.clear();
        const int st = adaptive_params_check(&ap, p, npix);
        std::printf("  %s\n", g_err.c_str());
        return st == status && g_err.find(with) != std::string::npos;
    };
    RtAdaptiveParams ap = a.ap;
    ap.threshold = 0.0;
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "threshold must be positive and finite"));
    ap.threshold = std::numeric_limits<double>::quiet_NaN();
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "threshold must be positive and finite"));
    ap = a.ap; ap.floor = 0.0;
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "floor must be positive and finite"));
    ap = a.ap; ap.min_replicas = 1;
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "min_replicas must be at least 2"));
    ap = a.ap; ap.check_interval = 0;
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "check_interval must be at least 1"));
    ap = a.ap; ap.radius = 5;
    CHECK(refuses(ap, params, 6, RT_E_INVALID, "radius must be in 0 .. 4"));
    RtRenderParams parted = params;
    parted.band_rows = 1; parted.n_parts = 2;
    CHECK(refuses(a.ap, parted, 6, RT_E_INVALID, "row partition"));
    RtRenderParams flat = params;
    flat.max_depth = 0;
    CHECK(refuses(a.ap, flat, 6, RT_E_UNSUPPORTED, "max_depth = 0"));
    CHECK(refuses(a.ap, params, 1ull << 31, RT_E_UNSUPPORTED, "more than 2^31 pixels"));
    ap = a.ap; ap.threshold = 0.0; ap.radius = 5;  // the earlier check's message
    CHECK(refuses(ap, flat, 6, RT_E_INVALID, "threshold must be positive and finite"));
    return 0;
}

static int check_noise() {
    CHECK(accum_noise(3.0, 9.0, 0, 0.01) == 0.0 && accum_noise(3.0, 9.0, 1, 0.01) == 0.0);
    CHECK(accum_noise(4.0, 3.0, 4, 0.01) == 0.0);  // s2 - s1^2 / k = 3 - 4 < 0: clamped
    // k = 2, luminances 1 and 3: s1 = 4, s2 = 10, mean 2, numerator 10 - 8 = 2, se = sqrt(2 / (2 * 1)) = 1, floor 0.5: 1 / 2.5
    CHECK(accum_noise(4.0, 10.0, 2, 0.5) == 0.4);
    std::printf("noise: k < 2 gives 0, a negative numerator clamps to 0, (s1 4, s2 10, k 2, floor 0.5) gives %.17g\n", accum_noise(4.0, 10.0, 2, 0.5));
    return 0;
}

static int check_frame_digest() {
    RtCameraDesc cam{};
    cam.image_width = 3; cam.image_height = 2;
    RtRenderParams p{};
    p.sqrt_spt = 4; p.thread_count = 6; p.max_depth = 8; p.seed = 7;
    RtRenderParams q = p;
    q.pipeline = RT_PIPELINE_WAVEFRONT; q.collect_stats = 1;
    CHECK(frame_digest(cam, p) == frame_digest(cam, q));  // pipeline and collect_stats do not change the frame
    q = p; q.seed = 8;
    CHECK(frame_digest(cam, p) != frame_digest(cam, q));
    q = frame_fields(p);
    CHECK(q.pipeline == 0 && q.collect_stats == 0 && q.seed == p.seed);
    std::printf("frame digest: pipeline and collect_stats ignored, seed not\n");
    return 0;
}

int main() {
    if (check_corruptions() || check_lengths(fields(false, 4)) || check_lengths(fields(true, 4)) || check_counts() || check_schedule() ||
        check_adaptive_params() || check_noise() || check_frame_digest())
        return 1;
    std::printf("ok\n");
    return 0;
}
