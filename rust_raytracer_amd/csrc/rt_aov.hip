// rt_aov.hip — first-hit AOV pass and the edge-avoiding a-trous denoiser (include/rt_mi355.h: rt_render_aov,
// rt_denoise), with the denoiser's entry points.  A translation unit of its own: the render kernels in
// rt_kernels.hip are not touched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "rt_aov.h"
#include "rt_device.h"

namespace rt {

// ---------------------------------------------------------------------------------------------
// First-hit AOVs.  The megakernel's tiling (one lane per pixel, 16x16 tiles, the row partition through row_to_y) and its
// sample order (replica t, then stratum sy, sx).  Every sample is keyed, its camera ray built and its closest hit found
// exactly as k_megakernel does it: the same RNG key, get_ray, world_test with the path's RNG (so a volume draws as in
// the render) and resolve_hit.  No bounce is traced.  Per replica the S^2 samples are summed, then the replica's sum /
// (r S^2) is added in replica order, like the frame's sums.
// ---------------------------------------------------------------------------------------------
template <typename R, bool TEX>
__global__ void __launch_bounds__(256) k_aov(SceneView<R> sc, CameraView<R> cam, ParamsView<R> prm, uint32_t n_rep,
                                             double* __restrict__ out) {
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
    const double n_samples = double(per_replica) * double(n_rep);
    const uint64_t pixel_index = uint64_t(py) * cam.width + px;
    LaneCounters cnt;
    double acc[kAovChannels] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t t = 0; t < n_rep; t++) {
        double col[kAovChannels] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t st = 0; st < per_replica; st++) {
            const uint32_t sy = st / S, sx = st - sy * S;
            Rng rng;
            rng.key(prm.seed, t, pixel_index, st);
            const Ray<R> ray = get_ray(cam, px, py, sx, sy, rng);
            Best<R> best;
            world_test<R, false, TEX>(sc, ray, R(0.001), best, stack, stride, cnt, &rng);
            V3<R> albedo = ld3(prm.background);  // a miss: the background (0 without one), camera.rs:331
            V3<R> normal = mk<R>(0, 0, 0);
            R depth = R(0), coverage = R(0);
            if (best.pc >= 0) {
                const HitInfo<R> hit = resolve_hit<R, TEX>(sc, ray, best);
                switch (sc.materials[hit.material].type) {
                    case RT_MAT_EMISSIVE: albedo = hit.front_face ? hit.tex_a : mk<R>(0, 0, 0); break;  // what it emits
                    case RT_MAT_NORMAL_DEBUG: albedo = hit.normal * R(0.5) + mk<R>(R(0.5), R(0.5), R(0.5)); break;
                    case RT_MAT_DIELECTRIC: albedo = mk<R>(1, 1, 1); break;
                    default: albedo = hit.tex_a; break;  // Lambertian, Metal, Glossy, Isotropic
                }
                const uint32_t op = sc.ops[best.pc].type;
                if (op != OP_SKY && op != OP_SUN) {  // the environment has no normal, depth or coverage
                    normal = hit.normal;
                    depth = length(hit.pos - ray.o);
                    coverage = R(1);
                }
            }
            col[0] += double(albedo.x); col[1] += double(albedo.y); col[2] += double(albedo.z);
            col[3] += double(normal.x); col[4] += double(normal.y); col[5] += double(normal.z);
            col[6] += double(depth);
            col[7] += double(coverage);
        }
        for (uint32_t k = 0; k < kAovChannels; k++) acc[k] += col[k] / n_samples;
    }
    double* o = out + (size_t(row) * cam.width + px) * kAovChannels;
    for (uint32_t k = 0; k < kAovChannels; k++) o[k] = acc[k];
}

template <typename R>
hipError_t aov_launch(const SceneView<R>& sc, const CameraView<R>& cam, const ParamsView<R>& prm, bool tex, uint32_t n_rep,
                      double* d_out, hipStream_t stream) {
    const uint32_t tiles_x = (cam.width + 15u) / 16u, tiles_y = (prm.owned_rows + 15u) / 16u;
    if (tiles_x == 0 || tiles_y == 0) return hipSuccess;
    const dim3 grid(tiles_x * tiles_y), block(256);
    const size_t lds = size_t(sc.stack_entries) * 256 * sizeof(int);
    if (tex) hipLaunchKernelGGL((k_aov<R, true>), grid, block, lds, stream, sc, cam, prm, n_rep, d_out);
    else hipLaunchKernelGGL((k_aov<R, false>), grid, block, lds, stream, sc, cam, prm, n_rep, d_out);
    return hipGetLastError();
}
template hipError_t aov_launch<double>(const SceneView<double>&, const CameraView<double>&, const ParamsView<double>&, bool,
                                       uint32_t, double*, hipStream_t);
template hipError_t aov_launch<float>(const SceneView<float>&, const CameraView<float>&, const ParamsView<float>&, bool,
                                      uint32_t, double*, hipStream_t);

// ---------------------------------------------------------------------------------------------
// Edge-avoiding a-trous filter (Dammertz et al. 2010).  Weights in f32, sums in f64; tests/denoise_ref.py is the
// numpy restatement, operation for operation.
// ---------------------------------------------------------------------------------------------

// Packs the guides into f32 and demodulates the colour (c / albedo per channel where albedo > 1e-3).  Elementwise, so
// `col` may be `rgba`.
__global__ void __launch_bounds__(256) k_dn_prep(const double* rgba, const double* __restrict__ aov, uint64_t npix, uint32_t demod,
                                                 float4* __restrict__ guide_az, float4* __restrict__ guide_nc, double* col) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const double* a = aov + kAovChannels * i;
    const float4 az = make_float4(float(a[0]), float(a[1]), float(a[2]), float(a[6]));
    const float4 nc = make_float4(float(a[3]), float(a[4]), float(a[5]), float(a[7]));
    guide_az[i] = az;
    guide_nc[i] = nc;
    double c0 = rgba[4 * i], c1 = rgba[4 * i + 1], c2 = rgba[4 * i + 2];
    const double c3 = rgba[4 * i + 3];
    if (demod) {
        if (az.x > 1e-3f) c0 = c0 / double(az.x);
        if (az.y > 1e-3f) c1 = c1 / double(az.y);
        if (az.z > 1e-3f) c2 = c2 / double(az.z);
    }
    col[4 * i] = c0;
    col[4 * i + 1] = c1;
    col[4 * i + 2] = c2;
    col[4 * i + 3] = c3;
}

// One iteration: 5x5 B3-spline taps `step` pixels apart, one lane per pixel in 16x16 tiles.  `remod`: the last
// iteration multiplies the albedo back in.
__global__ void __launch_bounds__(256) k_dn_atrous(const double* __restrict__ in, const float4* __restrict__ guide_az,
                                                   const float4* __restrict__ guide_nc, uint32_t w, uint32_t h, uint32_t step,
                                                   float den_c, float den_n, float den_a, float sigma_z, uint32_t remod,
                                                   double* __restrict__ out) {
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const size_t p = size_t(y) * w + x;
    const double c0 = in[4 * p], c1 = in[4 * p + 1], c2 = in[4 * p + 2], c3 = in[4 * p + 3];
    const bool centre_finite = isfinite(c0) && isfinite(c1) && isfinite(c2);
    const float f0 = float(c0), f1 = float(c1), f2 = float(c2);
    const float4 azp = guide_az[p], ncp = guide_nc[p];
    const float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, ws = 0.0;
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = int64_t(y) + int64_t(dy) * step;
        if (qy < 0 || qy >= int64_t(h)) continue;  // outside: skipped, not clamped
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = int64_t(x) + int64_t(dx) * step;
            if (qx < 0 || qx >= int64_t(w)) continue;
            const size_t q = size_t(qy) * w + size_t(qx);
            const double q0 = in[4 * q], q1 = in[4 * q + 1], q2 = in[4 * q + 2];
            if (!(isfinite(q0) && isfinite(q1) && isfinite(q2))) continue;
            const float4 azq = guide_az[q], ncq = guide_nc[q];
            float wc = 1.0f;
            if (centre_finite) {
                const float d0 = float(q0) - f0, d1 = float(q1) - f1, d2 = float(q2) - f2;
                wc = expf(-(d0 * d0 + d1 * d1 + d2 * d2) / den_c);
            }
            const float n0 = ncq.x - ncp.x, n1 = ncq.y - ncp.y, n2 = ncq.z - ncp.z;
            const float wn = expf(-(n0 * n0 + n1 * n1 + n2 * n2) / den_n);
            const float a0 = azq.x - azp.x, a1 = azq.y - azp.y, a2 = azq.z - azp.z;
            const float wa = expf(-(a0 * a0 + a1 * a1 + a2 * a2) / den_a);
            const float wz = expf(-fabsf(azq.w - azp.w) / (sigma_z * fmaxf(azp.w, azq.w) + 1e-30f));
            const float wt = kH[dy + 2] * kH[dx + 2] * wc * wn * wa * wz;
            if (!(wt > 0.0f)) continue;  // underflow, or a NaN guide
            const double wd = double(wt);
            s0 += wd * q0;
            s1 += wd * q1;
            s2 += wd * q2;
            ws += wd;
        }
    }
    double r0 = c0, r1 = c1, r2 = c2;  // no contributing tap: the pixel keeps its value
    if (ws > 0.0) {
        r0 = s0 / ws;
        r1 = s1 / ws;
        r2 = s2 / ws;
    }
    if (remod) {
        if (azp.x > 1e-3f) r0 = r0 * double(azp.x);
        if (azp.y > 1e-3f) r1 = r1 * double(azp.y);
        if (azp.z > 1e-3f) r2 = r2 * double(azp.z);
    }
    out[4 * p] = r0;
    out[4 * p + 1] = r1;
    out[4 * p + 2] = r2;
    out[4 * p + 3] = c3;
}

int denoise_scratch_reserve(DenoiseScratch& s, size_t npix) {
    if (s.npix >= npix && s.color) return RT_OK;
    s = DenoiseScratch{};
    const char* nomem = "denoiser scratch does not fit in device memory";
    int st = s.guide_az.reserve(npix * sizeof(float4), nomem);
    if (st == RT_OK) st = s.guide_nc.reserve(npix * sizeof(float4), nomem);
    if (st == RT_OK) st = s.color.reserve(npix * 4 * sizeof(double), nomem);
    if (st != RT_OK) s = DenoiseScratch{};
    else s.npix = npix;
    return st;
}

hipError_t denoise_launch(const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h, const RtDenoiseParams& dp,
                          double* d_out, DenoiseScratch& scratch, hipStream_t stream) {
    const size_t npix = size_t(w) * h;
    if (npix == 0) return hipSuccess;
    const uint32_t n = dp.iterations;
    if (n == 0) return d_out == d_rgba ? hipSuccess : hipMemcpyAsync(d_out, d_rgba, npix * 4 * sizeof(double), hipMemcpyDeviceToDevice, stream);
    if (scratch.npix < npix || !scratch.color) return hipErrorInvalidValue;
    // ping-pong between the scratch colour buffer and d_out, arranged so that iteration n - 1 writes d_out
    auto buf = [&](uint32_t i) { return (n - i) % 2 == 0 ? d_out : scratch.color.get(); };
    const uint32_t demod = (dp.flags & RT_DENOISE_DEMODULATE) ? 1u : 0u;
    hipLaunchKernelGGL(k_dn_prep, dim3(uint32_t((npix + 255) / 256)), dim3(256), 0, stream, d_rgba, d_aov, uint64_t(npix), demod,
                       scratch.guide_az.get(), scratch.guide_nc.get(), buf(0));
    const float sc = float(dp.sigma_color), sn = float(dp.sigma_normal), sa = float(dp.sigma_albedo), sz = float(dp.sigma_depth);
    const dim3 grid((w + 15u) / 16u, (h + 15u) / 16u);
    for (uint32_t i = 0; i < n; i++) {
        const float den_c = sc * sc * std::ldexp(1.0f, -int(i));  // sigma_c^2 2^-i (exact scaling by a power of two)
        hipLaunchKernelGGL(k_dn_atrous, grid, dim3(256), 0, stream, buf(i), scratch.guide_az.get(), scratch.guide_nc.get(), w, h, 1u << i,
                           den_c, sn * sn, sa * sa, sz, (i + 1 == n) ? demod : 0u, buf(i + 1));
    }
    return hipGetLastError();
}

// dp (NULL = the defaults) -> *out, checked.
int denoise_params(const RtDenoiseParams* dp, RtDenoiseParams* out, const char* who) {
    if (dp) *out = *dp;
    else rt_denoise_default_params(out);
    if (out->iterations > RT_DENOISE_MAX_ITERATIONS)
        return rt::set_err(RT_E_INVALID, std::string(who) + ": iterations must be at most " + std::to_string(RT_DENOISE_MAX_ITERATIONS));
    for (double sg : {out->sigma_color, out->sigma_normal, out->sigma_albedo, out->sigma_depth})
        if (!(sg > 0.0) || !std::isfinite(sg) || !std::isfinite(float(sg)) || !(float(sg) > 0.0f))
            return rt::set_err(RT_E_INVALID, std::string(who) + ": every sigma must be a positive, finite f32 number");
    return RT_OK;
}

// Runs the filter on HBM buffers of the current device and waits for it; scratch: the caller's, or (NULL) one of its own.
int denoise_run(const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h, const RtDenoiseParams& dp,
                double* d_out, rt::DenoiseScratch* scratch, hipStream_t stream) {
    using namespace rt;
    DenoiseScratch own;
    DenoiseScratch& scr = scratch ? *scratch : own;
    if (dp.iterations)
        if (int st = denoise_scratch_reserve(scr, size_t(w) * h)) return st;
    hipError_t e = denoise_launch(d_rgba, d_aov, w, h, dp, d_out, scr, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("denoise: ") + hipGetErrorString(e));
    return RT_OK;
}

}  // namespace rt

extern "C" {

int rt_denoise_default_params(RtDenoiseParams* out) {
    if (!out) return rt::set_err(RT_E_INVALID, "rt_denoise_default_params: NULL argument");
    *out = RtDenoiseParams{};
    out->iterations = 4;  // tuned on 1-replica estimates against the full frame
    out->aov_replicas = 1;
    out->flags = RT_DENOISE_DEMODULATE;
    out->sigma_color = 8.0;
    out->sigma_normal = 0.3;
    out->sigma_albedo = 0.3;
    out->sigma_depth = 0.1;
    return RT_OK;
}

int rt_denoise_device(int device, const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h, const RtDenoiseParams* dp,
                      double* d_rgba_out, void* stream) {
    using namespace rt;
    if (!d_rgba || !d_aov || !d_rgba_out) return set_err(RT_E_INVALID, "rt_denoise_device: NULL argument");
    RtDenoiseParams p;
    if (int v = denoise_params(dp, &p, "rt_denoise_device")) return v;
    HIP_TRY(hipSetDevice(device));
    return denoise_run(d_rgba, d_aov, w, h, p, d_rgba_out, nullptr, static_cast<hipStream_t>(stream));
}

int rt_denoise(int device, const double* rgba, const double* aov, uint32_t w, uint32_t h, const RtDenoiseParams* dp, double* rgba_out) {
    using namespace rt;
    if (!rgba || !aov || !rgba_out) return set_err(RT_E_INVALID, "rt_denoise: NULL argument");
    RtDenoiseParams p;
    if (int v = denoise_params(dp, &p, "rt_denoise")) return v;
    const size_t npix = size_t(w) * h;
    if (npix == 0) return RT_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> d_rgba, d_aov;
    if (int st = d_rgba.reserve(npix * 4 * sizeof(double))) return st;
    if (int st = d_aov.reserve(npix * kAovChannels * sizeof(double))) return st;
    HIP_TRY(hipMemcpy(d_rgba, rgba, npix * 4 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_aov, aov, npix * kAovChannels * sizeof(double), hipMemcpyHostToDevice));
    if (int st = denoise_run(d_rgba, d_aov, w, h, p, d_rgba, nullptr, nullptr)) return st;  // in place
    HIP_TRY(hipMemcpy(rgba_out, d_rgba, npix * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
