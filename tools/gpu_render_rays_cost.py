"""What a ray table costs against a camera (rt_render_rays).

    timeout -k 10 900 python tools/gpu_render_rays_cost.py --parent=<librt_mi355.so of the parent commit> [--steps=5] [--precision=f64]

C4 (bench.py's workload: scenes/cornell_dragon 1200 x 1200, 10 replicas of 10 x 10 strata) in ONE process, both libraries
loaded side by side as tools/gpu_fused_prims_ab.py loads them:
    parent, rt_render_device          the frame, by the parent commit's library
    this commit, rt_render_device     the same frame by this library (must equal the parent's bit for bit)
    this commit, rt_render_rays_device  the rays through the pixel centres of the same camera (first_pixel + x pdu + y pdv -
                                      position from position, row-major: the camera's own ray of a one-stratum sample without
                                      its jitter), with the same S, T, depth, bias and seed: the same number of samples,
                                      every one of a pixel along the same ray.  The table is in HBM (48 B per ray).
After one untimed warm-up round the sides alternate, `steps` timed calls each.  Per side: median / min / max wall time, Msamples/s
and the HIP-event sums of the kernels (rt_get_stats).  The frames of the third side are not the camera's (no jitter, no lens):
what is compared is the time of the same kernels on the same number of paths."""
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


def centre_rays(cam):
    """(origins, dirs), (W * H, 3) each: the --pick ray of every pixel, row-major."""
    W, H = cam.image_width, cam.image_height
    pos, fp = np.array(list(cam.position)), np.array(list(cam.first_pixel))
    pdu, pdv = np.array(list(cam.pixel_delta_u)), np.array(list(cam.pixel_delta_v))
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = fp + x[..., None] * pdu + y[..., None] * pdv - pos
    o = np.broadcast_to(pos, d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))


def main():
    opt = {"parent": "", "steps": "5", "precision": "f64"}
    for a in sys.argv[1:]:
        k, _, v = a.lstrip("-").partition("=")
        opt[k] = v
    if not os.path.exists(opt["parent"]):
        raise SystemExit("--parent=<device library of the parent commit> is required")
    steps = max(5, int(opt["steps"]))
    old = load_api("parent", os.path.abspath(opt["parent"]))
    new = load_api("new", os.path.join(REPO, "rust_raytracer_amd", "librt_mi355.so"))
    args = list(bench.WORKLOADS["c4"][0])
    args[0] = bench.ensure_dragon()
    args += ["--seed=1", f"--precision={opt['precision']}", "--pipeline=auto"]
    sides = []
    for name, api in (("parent, rt_render_device", old), ("this commit, rt_render_device", new)):
        hs = api.HostScene(args)
        sc = api.DeviceScene(hs.desc, 0)
        out = torch.empty((hs.height, hs.width, 4), dtype=torch.float64, device="cuda:0")
        sides.append([name, hs, hs.params.copy(), sc, out])
    _, hs, p, sc, _ = sides[1]
    W, H = hs.width, hs.height
    o, d = centre_rays(hs.camera)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_rays_out = torch.empty((H * W, 4), dtype=torch.float64, device="cuda:0")
    sides.append(["this commit, rt_render_rays_device", hs, p, sc, d_rays_out])
    samples = W * H * hs.spp
    print(f"c4 {W}x{H} @{hs.spp}spp {opt['precision']} = {samples / 1e6:.0f} Msamples per call; {steps} timed calls per side after one "
          f"warm-up round, sides alternating in one process", flush=True)
    rows = {s[0]: [] for s in sides}
    same = True
    for rep in range(steps + 1):
        for k, (name, hs_, p_, sc_, out) in enumerate(sides):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if k < 2:
                sc_.render_device(hs_.camera, p_, out.data_ptr())
            else:
                sc_.render_rays_device(W * H, d_o.data_ptr(), d_d.data_ptr(), p_, out.data_ptr())
            wall = 1e3 * (time.perf_counter() - t)
            st = sc_.stats()
            assert st.samples == samples, (name, st.samples)
            if k == 1:
                same = same and bool(torch.equal(out.view(torch.int64), sides[0][4].view(torch.int64)))
            if rep:
                rows[name].append((wall, st.kernel_ms, st.prims_kernel_ms, st.traversal_kernel_ms, st.shade_kernel_ms, st.n_launches, st.n_iterations))
    base = None
    for name, *_ in sides:
        a = np.array(rows[name])
        med = np.median(a, axis=0)
        base = med if base is None else base
        print(f"{name:36s} wall median {med[0]:8.2f} ms (min {a[:, 0].min():.2f}, max {a[:, 0].max():.2f}; {100 * (med[0] / base[0] - 1):+.2f} %) = "
              f"{samples / med[0] / 1e3:6.0f} Msamples/s | kernels {med[1]:8.2f} ms: prims {med[2]:6.1f}, traversal {med[3]:6.1f}, shade {med[4]:6.1f}, "
              f"rest {med[1] - med[2] - med[3] - med[4]:5.1f} | {int(med[5])} search launches in {int(med[6])} iterations", flush=True)
    rays = sides[2][4].cpu().numpy()
    frame = sides[1][4].cpu().numpy().reshape(-1, 4)
    print(f"this commit's frame equals the parent's bit for bit: {same}; mean radiance: frame {frame[:, :3].mean():.6f}, ray table {rays[:, :3].mean():.6f} "
          f"(pixel centres, no jitter: close, not equal)", flush=True)


if __name__ == "__main__":
    main()
