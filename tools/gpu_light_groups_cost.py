"""What light groups cost (rt_render_light_groups).

C4 (bench.py's workload) in one process: rt_render_device against rt_render_light_groups_device with the automatic
assignment (G = 3 there: unlit, the lamp, the background) and with the same table declared as G = 8 and G = 16 (the extra
groups are empty: the resolve kernel's work depends on G alone).  The four sides alternate after a warm-up round; per side
the median wall time of a step, the HIP-event times of the kernels (rt_get_stats: prims, traversal, shade, all kernels) and
of the two resolve kernels of a light-group render (RT_LG_LOG line of the library), the bytes the feature adds and the
device memory in use after the G = 16 render.  The frames are compared bit for bit with rt_render_device's.

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_light_groups_cost.py [--steps=N]   (N >= 5 timed steps per side, default 5)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, %r)
os.environ["RT_LG_LOG"] = "1"
import torch
import bench
from rust_raytracer_amd import api
steps = int(sys.argv[1])
args = list(bench.WORKLOADS["c4"][0])
args[0] = bench.ensure_dragon()
hs = api.HostScene(args)
p = hs.params.copy()
p.pipeline = api.RT_PIPELINE_WAVEFRONT
W, H, T, S2 = hs.width, hs.height, p.thread_count, p.sqrt_spt ** 2
samples = W * H * T * S2
sc = api.DeviceScene(hs.desc, 0)
auto = api.light_groups_auto(hs.desc, 16, bool(p.has_background))
sides = [("rt_render_device", None)] + [("light groups G = %%d" %% g, api.RtLightGroups.make(g, auto.table, auto.background_group, 0))
                                        for g in (auto.n_groups, 8, 16)]
d_frame = torch.empty((H, W, 4), dtype=torch.float64, device="cuda:0")
d_ref = torch.empty_like(d_frame)
d_groups = torch.empty((16, H, W, 4), dtype=torch.float64, device="cuda:0")
sc.render_device(hs.camera, p, d_ref.data_ptr())  # untimed: scene tables, pool, buffers
free0, total = torch.cuda.mem_get_info(0)
print("c4 %%dx%%d, %%d replicas of %%d strata = %%.0f Msamples per step; automatic assignment: %%d groups; %%d timed steps per side after one warm-up round"
      %% (W, H, T, S2, samples / 1e6, auto.n_groups, steps), flush=True)
rows = {name: [] for name, _ in sides}
same = True
for rep in range(steps + 1):
    for name, g in sides:
        torch.cuda.synchronize()
        t = time.perf_counter()
        if g is None:
            sc.render_device(hs.camera, p, d_frame.data_ptr())
        else:
            sc.render_light_groups_device(hs.camera, p, g, d_groups.data_ptr(), d_frame.data_ptr())
        wall = 1e3 * (time.perf_counter() - t)
        st = sc.stats()
        same = same and bool(torch.equal(d_frame.view(torch.int64), d_ref.view(torch.int64)))
        if rep:
            rows[name].append((wall, st.kernel_ms, st.prims_kernel_ms, st.traversal_kernel_ms, st.shade_kernel_ms))
        if g is not None and g.n_groups == 16 and rep == steps:
            free1, _ = torch.cuda.mem_get_info(0)
            print("device memory in use after the G = 16 render: %%.2f GB of %%.0f GB (%%.2f GB more than after rt_render_device: "
                  "group bytes %%.2f GB, nothing else is kept; the caller's 16 group frames are %%.2f GB)"
                  %% ((total - free1) / 2**30, total / 2**30, (free0 - free1) / 2**30, samples / 2**30, 16 * W * H * 32 / 2**30), flush=True)
base = None
for name, g in sides:
    a = np.array(rows[name])
    med = np.median(a, axis=0)
    if base is None:
        base = med
    print("%%-22s wall median %%8.1f ms (min %%.1f, max %%.1f; %%+.2f %%%%) = %%6.0f Msamples/s | kernels %%8.1f ms: prims %%6.1f, traversal %%6.1f, "
          "shade %%6.1f (%%+.2f %%%%), rest %%6.1f" %% (name, med[0], a[:, 0].min(), a[:, 0].max(), 100 * (med[0] / base[0] - 1), samples / med[0] / 1e3,
          med[1], med[2], med[3], med[4], 100 * (med[4] / base[4] - 1), med[1] - med[2] - med[3] - med[4]), flush=True)
print("the frame of every light-group render is rt_render_device's, bit for bit: %%s" %% same, flush=True)
print("added per sample: 1 B written by k_wf_shade, read G/4-fold ... G-fold by k_wf_resolve_groups (see the resolve times); "
      "per pixel: G x 32 B of output, and G x 24 B of running sums when the replicas do not fit one group", flush=True)
''' % (REPO,)

steps = 5
for a in sys.argv[1:]:
    if a.startswith("--steps="):
        steps = max(5, int(a.split("=", 1)[1]))
r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", CODE, str(steps)], capture_output=True, text=True)
sys.stdout.write(r.stdout)
res = {}
for ln in r.stderr.splitlines():  # "[light groups] G 16: resolve kernels 12.345 ms, ..."
    if ln.startswith("[light groups] G "):
        g = int(ln.split()[3].rstrip(":"))
        res.setdefault(g, []).append(float(ln.split("resolve kernels")[1].split("ms")[0]))
for g, ms in sorted(res.items()):
    ms = sorted(ms[1:])  # without the warm-up round
    print(f"G = {g:2d}: k_wf_resolve + k_wf_resolve_groups median {ms[len(ms) // 2]:.2f} ms per step (min {ms[0]:.2f}, max {ms[-1]:.2f})")
if r.returncode != 0:
    sys.stdout.write(r.stderr[-3000:])
    print(f"exit status {r.returncode}: stopping")
    sys.exit(1)
