"""What adaptive sampling costs and saves (rt_accum_set_adaptive).

  optin     C4 (bench.py's workload: 10 replicas) in passes of 10, 5 and 2 replicas: a plain accumulator against an adaptive
            one WITHOUT a decision point (min_replicas = T: only the moments in the resolve step differ), alternating in one
            process after a warm-up, several repeats each; the frames compared bit for bit.  With --parent-lib=<path of a
            librt_mi355.so built from the parent commit> that library's plain accumulator is a third side of the rotation.
  sparse    C4 and C2 at 40 replicas with the default rule at a threshold: every pass (check_interval replicas) with its
            active share, samples, wall and kernel time -> Msamples/s of the dense passes (before the first pixel stops)
            and of the sparse ones; the same frame in plain passes of the same size gives the per-pass cost without
            decisions, and one plain call the cost without the drain every pass adds.
  endtoend  C4 at 40 replicas of 5 x 5 strata at two thresholds: samples rendered, pixels stopped, wall time against the
            plain frame, and dev = |Y_adaptive - Y_full| / (Y_full + 0.01) over the stopped pixels.

Each measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends
the run (no further GPU work after a hang).  Usage: python tools/gpu_adaptive_cost.py [--parent-lib=PATH] [optin] [sparse] [endtoend]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import ctypes as C, sys, time
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import bench
import adaptive_ref as ar
from rust_raytracer_amd import api
which, parent_lib = sys.argv[1], sys.argv[2]
WAVE = api.RT_PIPELINE_WAVEFRONT

def workload(name, t=None, s=None):
    args = list(bench.WORKLOADS[name][0])
    if name == "c4":
        args[0] = bench.ensure_dragon()
    if t is not None:
        args = [a for a in args if not a.startswith("-t=")] + ["-t=%%d" %% t]
    if s is not None:
        args = [a for a in args if not a.startswith("-s=")] + ["-s=%%d" %% s]
    hs = api.HostScene(args)
    p = hs.params.copy()
    p.pipeline = WAVE
    return hs, p

def passes(pr, n):
    t = time.perf_counter()
    while not pr.finished:
        pr.render(n)
    return 1e3 * (time.perf_counter() - t)

class ParentAccum:
    """The plain accumulator of another build of the library, through its own handle (rt_accum_* as in api.py)."""
    def __init__(self, path, hs, p):
        lib = C.CDLL(path)
        lib.rt_scene_create.argtypes = [C.POINTER(api.RtSceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        lib.rt_accum_create.argtypes = [C.c_void_p, C.POINTER(api.RtCameraDesc), C.POINTER(api.RtRenderParams), C.POINTER(C.c_void_p)]
        lib.rt_accum_render.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(api.RtRenderParams), C.c_void_p]
        lib.rt_accum_replicas_done.argtypes = [C.c_void_p]
        lib.rt_accum_replicas_done.restype = C.c_uint32
        lib.rt_accum_estimate.argtypes = [C.c_void_p, C.c_void_p]
        lib.rt_accum_destroy.argtypes = [C.c_void_p]
        lib.rt_last_error.restype = C.c_char_p
        self.lib, self.hs, self.p = lib, hs, p
        self.scene = C.c_void_p()
        assert lib.rt_scene_create(hs.desc, 0, C.byref(self.scene)) == 0, lib.rt_last_error()
    def frame(self, n):
        lib, acc = self.lib, C.c_void_p()
        assert lib.rt_accum_create(self.scene, C.byref(self.hs.camera), C.byref(self.p), C.byref(acc)) == 0, lib.rt_last_error()
        t = time.perf_counter()
        while lib.rt_accum_replicas_done(acc) < self.p.thread_count:
            assert lib.rt_accum_render(acc, n, None, None) == 0, lib.rt_last_error()
        ms = 1e3 * (time.perf_counter() - t)
        out = np.empty((self.hs.height, self.hs.width, 4))
        assert lib.rt_accum_estimate(acc, out.ctypes.data) == 0
        lib.rt_accum_destroy(acc)
        return ms, out

if which == "optin":
    hs, p = workload("c4")
    T = p.thread_count
    sc = api.DeviceScene(hs.desc, 0)
    one = sc.render(hs.camera, p)  # untimed: scene tables, pool, buffers
    off = api.RtAdaptiveParams.defaults(threshold=0.1, min_replicas=T)  # no decision point
    parent = ParentAccum(parent_lib, hs, p) if parent_lib else None
    def plain(n):
        pr = api.ProgressiveRender(sc, hs.camera, p)
        ms = passes(pr, n)
        out = pr.estimate(); pr.close()
        return ms, out
    def adaptive(n):
        pr = api.ProgressiveRender(sc, hs.camera, p, adaptive=off)
        ms = passes(pr, n)
        out = pr.estimate(); pr.close()
        return ms, out
    sides = [("plain", plain), ("adaptive, no decision point", adaptive)] + ([("parent's plain", parent.frame)] if parent else [])
    for n in (10, 5, 2):
        times = {name: [] for name, _ in sides}
        same = True
        for rep in range(6):  # the first round of each side is the warm-up
            for name, f in sides:
                ms, out = f(n)
                same = same and bool((out.view(np.uint64) == one.view(np.uint64)).all())
                if rep:
                    times[name].append(ms)
        base = float(np.median(times["parent's plain" if parent else "plain"]))
        for name, _ in sides:
            ts = times[name]
            print("passes of %%2d: %%-28s median %%.1f ms (min %%.1f, max %%.1f; %%+.2f %%%% against %%s)" %% (
                n, name, np.median(ts), min(ts), max(ts), 100 * (np.median(ts) / base - 1), "the parent" if parent else "plain"), flush=True)
        print("passes of %%2d: every frame bit-identical to rt_render's: %%s" %% (n, same), flush=True)
elif which == "sparse":
    for name, thr in (("c4", 0.1), ("c2", 0.1)):
        hs, p = workload(name, t=40, s=1000 if name == "c4" else 640)
        T, S2, npix = p.thread_count, p.sqrt_spt ** 2, hs.width * hs.height
        sc = api.DeviceScene(hs.desc, 0)
        t = time.perf_counter(); sc.render(hs.camera, p); sc.render(hs.camera, p)
        t = time.perf_counter(); sc.render(hs.camera, p)
        one_ms = 1e3 * (time.perf_counter() - t)
        ap = api.RtAdaptiveParams.defaults(threshold=thr)
        n = ap.check_interval
        pr = api.ProgressiveRender(sc, hs.camera, p)
        plain_walls = []
        while not pr.finished:
            ts = time.perf_counter(); pr.render(n); plain_walls.append(1e3 * (time.perf_counter() - ts))
        pr.close()
        dense_pass = float(np.median(plain_walls[1:]))
        print("%%s %%dx%%d, %%d replicas of %%d: one call %%.1f ms = %%.0f Msamples/s; plain passes of %%d: %%.1f ms each = %%.0f Msamples/s "
              "(%%.1f ms per pass more than its share of the one call)" %% (name, hs.width, hs.height, T, S2, one_ms, npix * S2 * T / one_ms / 1e3, n,
              dense_pass, npix * S2 * n / dense_pass / 1e3, dense_pass - one_ms * n / T), flush=True)
        for rep in range(2):
            pr = api.ProgressiveRender(sc, hs.camera, p, adaptive=ap)
            rows = []
            while not pr.finished:
                active = pr.active_pixels
                ts = time.perf_counter(); pr.render(n); wall = 1e3 * (time.perf_counter() - ts)
                st = sc.stats()
                rows.append((pr.replicas_done, active / npix, st.samples, wall, st.kernel_ms))
            if rep:  # the second run is the record
                for k, share, samples, wall, kms in rows:
                    print("  %%s adaptive pass to k = %%2d: %%5.1f %%%% active, %%6.1f Msamples, %%6.1f ms wall (%%6.1f ms kernels) = %%5.0f Msamples/s; "
                          "the dense pass costs %%.1f ms, this share of it %%.1f ms" %% (name, k, 100 * share, samples / 1e6, wall, kms,
                          samples / wall / 1e3, dense_pass, dense_pass * share), flush=True)
            pr.close()
elif which == "endtoend":
    hs, p = workload("c4", t=40)
    T, npix = p.thread_count, hs.width * hs.height
    sc = api.DeviceScene(hs.desc, 0)
    sc.render(hs.camera, p)
    t = time.perf_counter(); full = sc.render(hs.camera, p); full_ms = 1e3 * (time.perf_counter() - t)
    print("c4 %%d replicas of %%d: plain frame %%.1f ms" %% (T, p.sqrt_spt ** 2, full_ms), flush=True)
    for thr, ci in ((0.1, 2), (0.05, 2), (0.1, 4), (0.1, 8)):
        ap = api.RtAdaptiveParams.defaults(threshold=thr, check_interval=ci)
        walls = []
        for rep in range(3):
            pr = api.ProgressiveRender(sc, hs.camera, p, adaptive=ap)
            t = time.perf_counter(); pr.render(T); walls.append(1e3 * (time.perf_counter() - t))
            n, est, k = pr.sample_counts(), pr.estimate(), pr.replicas_done
            pr.close()
        q = ar.quality(est, full, n, T, thr)
        print("  threshold %%.2f, check_interval %%d: %%.1f %%%% of the pixels stopped, %%.1f %%%% of the samples rendered, k = %%d, wall %%.1f ms "
              "(median of 3; %%.1f %%%% of the plain frame), dev > thr on %%.2f %%%% and > 3 thr on %%.2f %%%% of the stopped pixels"
              %% (thr, ci, 100 * q["stopped"], 100 * q["rendered"], k, np.median(walls), 100 * np.median(walls) / full_ms, 100 * q["over"], 100 * q["over3"]), flush=True)
''' % (REPO, os.path.join(REPO, "tests"))

args = sys.argv[1:]
parent = ""
for a in list(args):
    if a.startswith("--parent-lib="):
        parent = os.path.abspath(a.split("=", 1)[1])
        args.remove(a)
for which in (args or ["optin", "sparse", "endtoend"]):
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", CODE, which, parent], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-3000:])
        print(f"[{which}] exit status {r.returncode}: stopping")
        sys.exit(1)
