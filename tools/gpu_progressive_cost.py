"""What progressive rendering costs (rt_accum_*, DESIGN.md "Progressive, resumable rendering").

  frames   C4 (bench.py's workload: 10 replicas) rendered one-shot and in passes of 5, 2 and 1 replicas (wavefront pipeline,
           the pool sized from the whole frame): wall time of the frame, sum of the calls' kernel time, and the result
           compared bit for bit with the one-shot frame
  preview  rt_accum_preview_rgb8 (estimate + output stage on the device, 3 B per pixel to the host) against
           rt_accum_estimate (32 B per pixel) + the host output stage (api.tonemap_rgb8), at 1200^2 and 2400^2

Each measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends
the run (no further GPU work after a hang).  Usage: python tools/gpu_progressive_cost.py [frames] [preview]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import sys, time
import numpy as np
sys.path.insert(0, %r)
import bench
from rust_raytracer_amd import api
which = sys.argv[1]
if which == "frames":
    bench.ensure_dragon()
    hs = api.HostScene(bench.WORKLOADS["c4"][0])
    p = hs.params.copy()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    sc = api.DeviceScene(hs.desc, 0)
    sc.render(hs.camera, p)  # untimed: scene tables, pool, buffers
    t = time.perf_counter()
    one = sc.render(hs.camera, p)
    print("one-shot: %%.1f ms wall, %%.1f ms kernels" %% (1e3 * (time.perf_counter() - t), sc.stats().kernel_ms), flush=True)
    for n in (5, 2, 1):
        pr = api.ProgressiveRender(sc, hs.camera, p)
        kms, walls = 0.0, []
        t = time.perf_counter()
        while pr.replicas_done < p.thread_count:
            ts = time.perf_counter()
            pr.render(n)
            walls.append(1e3 * (time.perf_counter() - ts))
            kms += sc.stats().kernel_ms
        wall = 1e3 * (time.perf_counter() - t)
        same = bool((pr.estimate().view(np.uint64) == one.view(np.uint64)).all())
        print("passes of %%d: %%d passes, %%.1f ms wall, %%.1f ms kernels, pass walls %%s ms, bit-identical %%s"
              %% (n, len(walls), wall, kms, " ".join("%%.1f" %% w for w in walls), same), flush=True)
        pr.close()
else:
    for w in (1200, 2400):
        hs = api.HostScene(["scenes/cornell", "-w=%%d" %% w, "-r=1", "-s=2", "-t=2", "--max-depth=2", "--seed=3"])
        sc = api.DeviceScene(hs.desc, 0)
        pr = api.ProgressiveRender(sc, hs.camera, hs.params)
        pr.render(1)
        def med(f, reps=7):
            f()
            ts = []
            for _ in range(reps):
                t = time.perf_counter(); f(); ts.append(1e3 * (time.perf_counter() - t))
            return float(np.median(ts))
        dev = med(pr.preview_rgb8)
        host_est = med(pr.estimate)
        est = pr.estimate()
        host_tm = med(lambda: api.tonemap_rgb8(est))
        print("%%dx%%d: preview_rgb8 %%.2f ms; estimate %%.2f ms + host tonemap %%.2f ms = %%.2f ms; bytes equal %%s"
              %% (w, w, dev, host_est, host_tm, host_est + host_tm, bool((pr.preview_rgb8() == api.tonemap_rgb8(est)).all())), flush=True)
''' % REPO

for which in (sys.argv[1:] or ["frames", "preview"]):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", CODE, which], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-3000:])
        print(f"[{which}] exit status {r.returncode}: stopping")
        sys.exit(1)
