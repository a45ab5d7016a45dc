// The first rays of an irradiance bake (rt_bake_irradiance) computed on the HOST by the device's own code:
// the WfGroupPoints branch of wf_new_sample (rust_raytracer_amd/csrc/rt_wavefront.h) with the device functions compiled for the
// host as well.  No GPU is needed or touched.  tests/test_bake_irradiance_host.py builds it with the address and
// undefined-behaviour sanitizers and compares what it writes with the numpy restatement bit for bit:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//           -Xarch_host -fno-sanitize-recover=all -Iinclude -o point_ray_host tools/point_ray_host.cpp
// (the header also defines kernels, so the device side is compiled too, without sanitizers; the program launches nothing)
//     point_ray_host <in> <out>
// <in>:  u64 seed, u32 S, u32 T, u64 first, u32 n, u32 stride (24: positions then normals, n x 3 doubles each; 96: n RtRayHit
//        records), then the arrays.
// <out>: per point k, replica t, stratum st, in that order: o[3], d'[3] as doubles.
#define RT_DEV __host__ __device__ inline
#define RT_DEV_NOINLINE __host__ __device__ __attribute__((noinline))
#include "../rust_raytracer_amd/csrc/rt_wavefront.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    struct Header { uint64_t seed; uint32_t S, T; uint64_t first; uint32_t n, stride; } h;
    if (std::fread(&h, sizeof h, 1, f) != 1) return 2;
    const size_t bytes = h.stride == 24 ? size_t(h.n) * 48 : size_t(h.n) * h.stride;
    std::vector<unsigned char> data(bytes);
    if (bytes && std::fread(data.data(), 1, bytes, f) != bytes) return 2;
    std::fclose(f);
    using namespace rt;
    const uint32_t strata = h.S * h.S;
    WfGroupPoints<double> grp{};
    grp.npix = h.n;
    grp.per_replica = uint64_t(strata) * h.n;
    grp.total = grp.per_replica * h.T;
    grp.inv_per_replica = 1.0 / double(grp.per_replica);
    grp.inv_npix = 1.0 / double(grp.npix);
    grp.inv_width = 1.0 / double(h.n);
    grp.tid0 = 0;
    grp.strata = strata;
    grp.first = h.first;
    grp.stride = h.stride;
    grp.pos = data.data() + (h.stride == 24 ? 0 : offsetof(RtRayHit, pos));
    grp.nrm = data.data() + (h.stride == 24 ? size_t(h.n) * 24 : offsetof(RtRayHit, normal));
    CameraView<double> cam{};
    cam.sqrt_spt = h.S;
    cam.inv_sqrt_spt = 1.0 / double(h.S);
    cam.width = h.n;
    ParamsView<double> prm{};
    prm.seed = h.seed;
    std::FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 2;
    for (uint32_t k = 0; k < h.n; k++)
        for (uint32_t t = 0; t < h.T; t++)
            for (uint32_t st = 0; st < strata; st++) {
                V3<double> o, d;
                Rng rng;
                wf_new_sample((uint64_t(t) * strata + st) * h.n + k, grp, cam, prm, o, d, rng);
                const double row[6] = {o.x, o.y, o.z, d.x, d.y, d.z};
                std::fwrite(row, sizeof row, 1, g);
            }
    return std::fclose(g) == 0 ? 0 : 2;
}
