"""A/B of two device libraries in ONE process (fused k_wf_shade + k_wf_prims).

    timeout -k 10 900 python tools/gpu_fused_prims_ab.py --parent=<librt_mi355.so of the parent commit> [--workloads=c4,c2] [--steps=5]

Both libraries are loaded side by side (each through its own copy of rust_raytracer_amd/api.py, so that each has its own ctypes
binding), each renders bench.py's workload into its own device frame; after one untimed warm-up round the sides alternate, `steps`
timed frames each.  Per side: median / min / max wall time of a frame, the HIP-event sums of the kernels (rt_get_stats), and
whether every frame equals the parent's bit for bit.  `verdict` applies the criterion: the medians differ by more than three
times the larger min-max spread of the two sides.  Extra sides: --env=NAME=VALUE renders the new library once more with that
variable set (e.g. RT_WF_FUSE=0, the new library's own unfused pipeline); several variables of one side are joined with a
comma (--env=RT_WF_HANDOUT_256=512,RT_WF_HANDOUT_128=128)."""
import importlib.util
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402  (before the libraries: see api.load_device_lib)
import bench  # noqa: E402


def load_api(tag, lib_path):
    os.environ["RT_DEVICE_LIB"] = lib_path
    spec = importlib.util.spec_from_file_location(f"rt_api_{tag}", os.path.join(REPO, "rust_raytracer_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.load_device_lib()
    del os.environ["RT_DEVICE_LIB"]
    return mod


def main():
    opt = {"parent": "", "workloads": "c4", "steps": "5", "precision": "f64"}
    envs = []
    for a in sys.argv[1:]:
        k, _, v = a.lstrip("-").partition("=")
        if k == "env":
            envs.append((v, dict(kv.split("=", 1) for kv in v.split(","))))
        else:
            opt[k] = v
    if not os.path.exists(opt["parent"]):
        raise SystemExit("--parent=<device library of the parent commit> is required")
    steps = max(5, int(opt["steps"]))
    apis = {"parent": load_api("parent", os.path.abspath(opt["parent"])),
            "this commit": load_api("new", os.path.join(REPO, "rust_raytracer_amd", "librt_mi355.so"))}
    for wl in opt["workloads"].split(","):
        args = list(bench.WORKLOADS[wl][0])
        if wl == "c4":
            args[0] = bench.ensure_dragon()
        sides = []
        for name, api in apis.items():
            hs = api.HostScene(args + ["--seed=1", f"--precision={opt['precision']}", "--pipeline=auto"])
            p = hs.params.copy()
            sc = api.DeviceScene(hs.desc, 0)
            out = torch.empty((hs.height, hs.width, 4), dtype=torch.float64, device="cuda:0")
            sides.append([name, hs, p, sc, out, {}])
        for label, env in envs:
            n, hs, p, sc, _, _ = sides[1]
            sides.append([f"this commit, {label}", hs, p, sc, torch.empty_like(sides[1][4]), env])
        hs = sides[0][1]
        samples = hs.width * hs.height * hs.spp
        print(f"{wl} {hs.width}x{hs.height} @{hs.spp}spp {opt['precision']} = {samples / 1e6:.0f} Msamples per frame; {steps} timed frames per side "
              f"after one warm-up round, sides alternating in one process", flush=True)
        rows = {s[0]: [] for s in sides}
        same = {s[0]: True for s in sides}
        for rep in range(steps + 1):
            for name, hs_, p, sc, out, env in sides:
                for k, v in env.items():
                    os.environ[k] = v
                torch.cuda.synchronize()
                t = time.perf_counter()
                sc.render_device(hs_.camera, p, out.data_ptr())
                wall = 1e3 * (time.perf_counter() - t)
                for k in env:
                    del os.environ[k]
                st = sc.stats()
                same[name] = same[name] and bool(torch.equal(out.view(torch.int64), sides[0][4].view(torch.int64)))
                if rep:
                    rows[name].append((wall, st.kernel_ms, st.prims_kernel_ms, st.traversal_kernel_ms, st.shade_kernel_ms, st.n_launches, st.n_iterations))
        base = None
        res = {}
        for name, *_ in sides:
            a = np.array(rows[name])
            med = np.median(a, axis=0)
            base = med if base is None else base
            res[name] = (med[0], a[:, 0].min(), a[:, 0].max())
            print(f"{name:34s} wall median {med[0]:8.2f} ms (min {a[:, 0].min():.2f}, max {a[:, 0].max():.2f}; {100 * (med[0] / base[0] - 1):+.2f} %) = "
                  f"{samples / med[0] / 1e3:6.0f} Msamples/s | kernels {med[1]:8.2f} ms: prims {med[2]:6.1f}, traversal {med[3]:6.1f}, shade {med[4]:6.1f}, "
                  f"rest {med[1] - med[2] - med[3] - med[4]:5.1f} | {int(med[5])} search launches in {int(med[6])} iterations | "
                  f"frames equal the parent's bit for bit: {same[name]}", flush=True)
        (m0, lo0, hi0), (m1, lo1, hi1) = res["parent"], res["this commit"]
        spread = max(hi0 - lo0, hi1 - lo1)
        print(f"verdict {wl}: parent - this commit = {m0 - m1:+.2f} ms ({100 * (m0 - m1) / m0:+.2f} %); larger min-max spread {spread:.2f} ms "
              f"({100 * spread / m0:.2f} %); faster by more than 3 spreads: {m0 - m1 > 3 * spread}; slower by more than one spread: {m1 - m0 > spread}", flush=True)
        del sides
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
