// The first rays of a table mode computed on the HOST by the device's own code: the WfGroupPoints branch of wf_new_sample
// (rt_bake_irradiance) or its WfGroupProbes branch (rt_bake_probes, section 19), from
// rust_raytracer_amd/csrc/rt_wavefront.h with the device functions compiled for the host as well.  For probes also what
// k_wf_resolve_sh evaluates per sample - key, wf_strat_uniforms, wf_probe_dir, wf_sh_basis - for the nine Y_k.  No GPU is needed
// or touched.  tests/test_bake_irradiance_host.py and tests/test_bake_probes_host.py build it with the address and
// undefined-behaviour sanitizers and compare what it writes with the numpy restatement bit for bit:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//           -Xarch_host -fno-sanitize-recover=all -Iinclude -o table_ray_host tools/table_ray_host.cpp
// (the header also defines kernels, so the device side is compiled too, without sanitizers; the program launches nothing)
//     table_ray_host <in> <out>
// <in>:  u64 seed, u32 S, u32 T, u64 first, u32 n, u32 stride, then the arrays.  stride 24: points, positions then normals,
//        n x 3 doubles each; 96: points, n RtRayHit records; 0: probes, n x 3 doubles of positions.
// <out>: per entry k, replica t, stratum st, in that order, as doubles: o[3], d'[3], and for probes Y_0 .. Y_8.
#define RT_DEV __host__ __device__ inline
#define RT_DEV_NOINLINE __host__ __device__ __attribute__((noinline))
#include "../rust_raytracer_amd/csrc/rt_wavefront.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace rt;

struct Header { uint64_t seed; uint32_t S, T; uint64_t first; uint32_t n, stride; };

// `cols` doubles per sample of the table `grp` describes (everything but its pointers is filled here); extra(k, t, st, rng, row)
// fills what follows o and d' and may refuse (false).
template <typename G, typename F>
static int write_rows(const Header& h, G grp, const char* path, size_t cols, F&& extra) {
    const uint32_t strata = h.S * h.S;
    grp.npix = h.n;
    grp.per_replica = uint64_t(strata) * h.n;
    grp.total = grp.per_replica * h.T;
    grp.inv_per_replica = 1.0 / double(grp.per_replica);
    grp.inv_npix = 1.0 / double(grp.npix);
    grp.inv_width = 1.0 / double(h.n);
    grp.tid0 = 0;
    grp.strata = strata;
    grp.first = h.first;
    CameraView<double> cam{};
    cam.sqrt_spt = h.S;
    cam.inv_sqrt_spt = 1.0 / double(h.S);
    cam.width = h.n;
    ParamsView<double> prm{};
    prm.seed = h.seed;
    std::FILE* g = std::fopen(path, "wb");
    if (!g) return 2;
    for (uint32_t k = 0; k < h.n; k++)
        for (uint32_t t = 0; t < h.T; t++)
            for (uint32_t st = 0; st < strata; st++) {
                V3<double> o, d;
                Rng rng;
                wf_new_sample((uint64_t(t) * strata + st) * h.n + k, grp, cam, prm, o, d, rng);
                double row[15] = {o.x, o.y, o.z, d.x, d.y, d.z};
                if (!extra(k, t, st, rng, row)) return 3;
                std::fwrite(row, sizeof(double), cols, g);
            }
    return std::fclose(g) == 0 ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Header h;
    if (std::fread(&h, sizeof h, 1, f) != 1) return 2;
    const size_t bytes = size_t(h.n) * (h.stride == 0 ? 24 : h.stride == 24 ? 48 : h.stride);
    std::vector<double> data((bytes + 7) / 8);  // doubles: the probe positions are read as such
    if (bytes && std::fread(data.data(), 1, bytes, f) != bytes) return 2;
    std::fclose(f);
    if (h.stride == 0) {
        WfGroupProbes<double> grp{};
        grp.pos = data.data();
        const double inv_S = 1.0 / double(h.S);
        return write_rows(h, grp, argv[2], 15, [&](uint32_t k, uint32_t t, uint32_t st, const Rng& rng, double* row) {
            Rng again;  // the resolve's side: the direction from the key alone
            again.key(h.seed, t, h.first + k, st);
            double u1, u2;
            wf_strat_uniforms<double>(again, st, h.S, inv_S, u1, u2);
            if (again.s != rng.s) return false;  // both sides have drawn the same two uniforms
            const V3<double> dir = wf_probe_dir<double>(u1, u2);
            for (uint32_t c = 0; c < 9; c++) row[6 + c] = wf_sh_basis<double>(c, dir);
            return true;
        });
    }
    const unsigned char* base = reinterpret_cast<const unsigned char*>(data.data());
    WfGroupPoints<double> grp{};
    grp.stride = h.stride;
    grp.pos = base + (h.stride == 24 ? 0 : offsetof(RtRayHit, pos));
    grp.nrm = base + (h.stride == 24 ? size_t(h.n) * 24 : offsetof(RtRayHit, normal));
    return write_rows(h, grp, argv[2], 6, [](uint32_t, uint32_t, uint32_t, const Rng&, double*) { return true; });
}
