"""What the denoised previews cost (rt_render_aov, rt_accum_*_denoised; DESIGN.md "First-hit AOVs and the denoiser").

For C2 and C4 at bench.py's sizes, after one rendered replica:
  aov      the first-hit AOV pass of one replica (the accumulator's default, dp.aov_replicas = 1): wall time of rt_render_aov_device
           into a device buffer (the kernel dominates: S^2 primary rays per pixel through the render's traversal)
  preview  rt_accum_preview_denoised_rgb8 with the AOVs cached (estimate + the filter + device tone map + 3 B per
           pixel to the host) against rt_accum_preview_rgb8, and rt_denoise_device alone (prep + the default iterations), median of 7

Each workload runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run (no further GPU work after a hang).  Usage: python tools/gpu_denoise_cost.py [c2] [c4]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import sys, time
import numpy as np
import torch
torch.cuda.init()  # torch's runtime first, as bench.py does
sys.path.insert(0, %r)
import bench
from rust_raytracer_amd import api
which = sys.argv[1]
args = list(bench.WORKLOADS[which][0])
if which == "c4":
    args[0] = bench.ensure_dragon()
hs = api.HostScene(args)
p = hs.params
sc = api.DeviceScene(hs.desc, 0)
w, h, S = hs.width, hs.height, p.sqrt_spt
def med(f, reps=7):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); f(); ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts))
d_aov = torch.empty((h, w, 8), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
aov_ms = med(lambda: sc.render_aov_device(hs.camera, p, d_aov.data_ptr(), 1), reps=3)
print("%%s %%dx%%d: AOV pass of 1 replica (%%d spp, %%.0f M primary rays) %%.1f ms"
      %% (which, w, h, S * S, w * h * S * S / 1e6, aov_ms), flush=True)
pr = api.ProgressiveRender(sc, hs.camera, p)
pr.render(1)
pr.preview_rgb8_denoised()  # renders and caches the AOVs
den = med(pr.preview_rgb8_denoised)
plain = med(pr.preview_rgb8)
est_den = med(pr.estimate_denoised)
d_rgba = torch.from_numpy(pr.estimate()).to("cuda:0")
d_out = torch.empty_like(d_rgba)
torch.cuda.synchronize()
filt = med(lambda: api.denoise_device(d_rgba.data_ptr(), d_aov.data_ptr(), w, h, d_out.data_ptr()))
print("%%s %%dx%%d: preview_rgb8_denoised %%.2f ms (cached AOVs), preview_rgb8 %%.2f ms, estimate_denoised %%.2f ms, "
      "denoise_device alone %%.2f ms (%%d iterations, scratch allocated per call)"
      %% (which, w, h, den, plain, est_den, filt, api.RtDenoiseParams.defaults().iterations), flush=True)
''' % REPO

for which in (sys.argv[1:] or ["c2", "c4"]):
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", CODE, which], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-3000:])
        print(f"[{which}] exit status {r.returncode}: stopping")
        sys.exit(1)
