// rt_aov.h — launchers of the first-hit AOV pass (called by the C ABI in rt_kernels.hip) and of the a-trous denoiser, whose
// entry points are in rt_aov.hip itself and whose other caller is the accumulator (rt_accum.hip).  Definitions of the
// outputs: include/rt_mi355.h (rt_render_aov, RtDenoiseParams), DESIGN.md §10.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rt_mi355.h"
#include "rt_owned.h"
#include "rt_scene.h"

namespace rt {

constexpr uint32_t kAovChannels = 8;  // albedo rgb, normal xyz, depth, coverage

// The replicas [0, n_rep) of the frame `prm` describes -> d_out (owned_rows x width x 8 doubles).  `tex`: the
// full-feature variant (texture interpreter and volumes), chosen exactly as the render chooses it.  Enqueued on `stream`.
template <typename R>
hipError_t aov_launch(const SceneView<R>& sc, const CameraView<R>& cam, const ParamsView<R>& prm, bool tex, uint32_t n_rep,
                      double* d_out, hipStream_t stream);

// Device scratch of the denoiser for up to `npix` pixels: the packed guides and one colour buffer (the output buffer is
// the other one of the ping-pong pair).
struct DenoiseScratch {
    DevBuf<float4> guide_az;  // albedo rgb, depth
    DevBuf<float4> guide_nc;  // normal xyz, coverage
    DevBuf<double> color;     // 4 doubles per pixel
    size_t npix = 0;
};
// RT_OK, or RT_E_NOMEM / RT_E_DEVICE with the message set; a failure leaves the scratch empty.
int denoise_scratch_reserve(DenoiseScratch& s, size_t npix);

// d_rgba (w*h*4 doubles) guided by d_aov (w*h*8) -> d_out (w*h*4, may be d_rgba); dp already validated.  Enqueued on
// `stream`; the caller synchronises.
hipError_t denoise_launch(const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h, const RtDenoiseParams& dp,
                          double* d_out, DenoiseScratch& scratch, hipStream_t stream);

// dp (NULL = the defaults) -> *out, checked; `who` names the entry point in the message.
int denoise_params(const RtDenoiseParams* dp, RtDenoiseParams* out, const char* who);
// Runs the filter on HBM buffers of the current device and waits for it; scratch: the caller's, or (NULL) one of its own.
int denoise_run(const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h, const RtDenoiseParams& dp, double* d_out,
                DenoiseScratch* scratch, hipStream_t stream);

}  // namespace rt
