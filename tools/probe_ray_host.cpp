// The first rays and SH weights of a probe bake (rt_bake_probes) computed on the HOST by the device's own
// code: the WfGroupProbes branch of wf_new_sample (rust_raytracer_amd/csrc/rt_wavefront.h) for (o, d'), and what k_wf_resolve_sh
// evaluates per sample - key, wf_strat_uniforms, wf_probe_dir, wf_sh_basis - for the nine Y_k, with the device functions compiled
// for the host as well.  No GPU is needed or touched.  tests/test_bake_probes_host.py builds it with the address and
// undefined-behaviour sanitizers and compares what it writes with the numpy restatement bit for bit:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//           -Xarch_host -fno-sanitize-recover=all -Iinclude -o probe_ray_host tools/probe_ray_host.cpp
// (the header also defines kernels, so the device side is compiled too, without sanitizers; the program launches nothing)
//     probe_ray_host <in> <out>
// <in>:  u64 seed, u32 S, u32 T, u64 first, u32 n, u32 0, then n x 3 doubles of positions.
// <out>: per probe k, replica t, stratum st, in that order: o[3], d'[3], Y_0 .. Y_8 as doubles.
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
    struct Header { uint64_t seed; uint32_t S, T; uint64_t first; uint32_t n, pad; } h;
    if (std::fread(&h, sizeof h, 1, f) != 1) return 2;
    std::vector<double> pos(size_t(h.n) * 3);
    if (h.n && std::fread(pos.data(), sizeof(double), pos.size(), f) != pos.size()) return 2;
    std::fclose(f);
    using namespace rt;
    const uint32_t strata = h.S * h.S;
    WfGroupProbes<double> grp{};
    grp.npix = h.n;
    grp.per_replica = uint64_t(strata) * h.n;
    grp.total = grp.per_replica * h.T;
    grp.inv_per_replica = 1.0 / double(grp.per_replica);
    grp.inv_npix = 1.0 / double(grp.npix);
    grp.inv_width = 1.0 / double(h.n);
    grp.tid0 = 0;
    grp.strata = strata;
    grp.first = h.first;
    grp.pos = pos.data();
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
                double row[15] = {o.x, o.y, o.z, d.x, d.y, d.z};
                Rng again;  // the resolve's side: the direction from the key alone
                again.key(h.seed, t, h.first + k, st);
                double u1, u2;
                wf_strat_uniforms<double>(again, st, h.S, cam.inv_sqrt_spt, u1, u2);
                if (again.s != rng.s) return 3;  // both sides have drawn the same two uniforms
                const V3<double> dir = wf_probe_dir<double>(u1, u2);
                for (uint32_t c = 0; c < 9; c++) row[6 + c] = wf_sh_basis<double>(c, dir);
                std::fwrite(row, sizeof row, 1, g);
            }
    return std::fclose(g) == 0 ? 0 : 2;
}
