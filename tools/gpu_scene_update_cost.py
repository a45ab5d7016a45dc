"""What rt_scene_update costs and what a refitted tree costs afterwards.

The headline scene (bench.py's c4: cornell_dragon, 871 200 triangles) in one process.  The mesh is displaced smoothly in
numpy, by about 1 % and about 20 % of its extent.  Three ways to get from the scene as loaded to a first frame of the displaced
one, each timed until a 1-replica render has returned (the device tables of a fresh scene are built lazily, so only then are
the sides comparable), alternating, RUNS times each (>= 7), median and min - max:
  (a) rt_scene_update on the live scene (its total_ms and refit_kernel_ms are reported as well),
  (b1) rt_scene_destroy + rt_scene_create with the host's binned-SAH builder,
  (b2) the same with RT_SCENE_BVH_ON_DEVICE (LBVH).
(h) is the host share of (a) alone: rt_scene_update on a scene that has nothing on the device yet (structure check, bytewise
compare, recompile, host refit of the exact f64 tables, copy of the held description, digest).
Then (c): the headline render on the refitted scene against a fresh host-SAH scene of the same geometry, for both
amplitudes, with node visits per mesh ray from a separate collect_stats run.

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_scene_update_cost.py [--runs=N]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import os, sys, time
import numpy as np
sys.path.insert(0, %r)
import bench
from rust_raytracer_amd import api
runs = int(sys.argv[1])
args = list(bench.WORKLOADS["c4"][0])
args[0] = bench.ensure_dragon()
def load(amplitude):
    hs = api.HostScene(args)
    m = max((hs.desc.contents.meshes[i] for i in range(hs.desc.contents.n_meshes)), key=lambda m: m.n_triangles)
    if amplitude:
        v = np.ctypeslib.as_array(m.positions, shape=(m.n_positions, 3))   # the loader's own array: displaced in place
        ext = float((v.max(axis=0) - v.min(axis=0)).max())
        c = 0.5 * (v.max(axis=0) + v.min(axis=0))
        u = (v - c) * (2 * np.pi / ext)
        v += amplitude * ext * np.stack([np.sin(1.3 * u[:, 1] + 0.4), np.sin(1.1 * u[:, 2] + 1.7), np.sin(0.9 * u[:, 0] + 2.9)], axis=1)
    return hs, m.n_triangles
base, n_tris = load(0.0)
moved = {"1 %%": load(0.01)[0], "20 %%": load(0.20)[0]}
p = base.params.copy()
p.pipeline = api.RT_PIPELINE_WAVEFRONT
p1 = p.copy()
p1.thread_count = 1
W, H = base.width, base.height
samples = W * H * p.thread_count * p.sqrt_spt ** 2
print("c4 %%dx%%d, mesh of %%d triangles; %%d runs per side, alternating" %% (W, H, n_tris, runs), flush=True)

def first_frame_fresh(hs, on_device):
    flags = hs.desc.contents.flags
    hs.desc.contents.flags = flags | api.RT_SCENE_BVH_ON_DEVICE if on_device else flags & ~api.RT_SCENE_BVH_ON_DEVICE
    t = time.perf_counter()
    sc = api.DeviceScene(hs.desc, 0)
    sc.render(hs.camera, p1)
    ms = 1e3 * (time.perf_counter() - t)
    hs.desc.contents.flags = flags
    sc.close()
    return ms

live = api.DeviceScene(base.desc, 0)
live.render(base.camera, p1)       # untimed: tables, pool
cold = api.DeviceScene(base.desc, 0)   # never rendered: its updates are the host share
rows, host_share = {}, {}
for rep in range(runs + 1):        # round 0 warms up (first update of the mesh uploads its index arrays)
    for name, hs in moved.items():
        t = time.perf_counter()
        info = live.update(hs.desc)
        live.render(hs.camera, p1)
        a = 1e3 * (time.perf_counter() - t)
        assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == n_tris
        h = cold.update(hs.desc)["total_ms"]
        h_back = cold.update(base.desc)["total_ms"]
        if rep:
            host_share.setdefault(name, []).extend([h, h_back])
        b1 = first_frame_fresh(hs, False)
        b2 = first_frame_fresh(hs, True)
        t = time.perf_counter()
        back = live.update(base.desc)                     # and back: a second sample of (a) per round
        live.render(base.camera, p1)
        a_back = 1e3 * (time.perf_counter() - t)
        if rep:
            rows.setdefault(name, []).append((a, info["total_ms"], info["refit_kernel_ms"], b1, b2, a_back, back["total_ms"], back["refit_kernel_ms"],
                                              info["bytes_uploaded"]))
def line(label, x):
    print("    %%-58s median %%8.1f ms (min %%.1f, max %%.1f)" %% (label, np.median(x), x.min(), x.max()), flush=True)
for name, r in rows.items():
    r = np.array(r)
    print("displacement %%s of the extent, to the first 1-replica frame:" %% name)
    line("(a) rt_scene_update + render", r[:, 0])
    line("    of which rt_scene_update total_ms", r[:, 1])
    line("    of which refit_kernel_ms", r[:, 2])
    line("(a) back to the scene as loaded: update + render", r[:, 5])
    line("    of which rt_scene_update total_ms", r[:, 6])
    line("    of which refit_kernel_ms", r[:, 7])
    line("(h) host share: rt_scene_update, nothing on the device", np.array(host_share[name]))
    line("(b1) destroy + create, host binned SAH, + render", r[:, 3])
    line("(b2) destroy + create, RT_SCENE_BVH_ON_DEVICE, + render", r[:, 4])
    print("    bytes uploaded per update: %%.1f MB" %% (r[:, 8].max() / 1e6))
    worst_a, best_b = max(r[:, 0].max(), r[:, 5].max()), min(r[:, 3].min(), r[:, 4].min())
    print("    slowest (a) %%.1f ms vs fastest (b) %%.1f ms: %%s" %% (worst_a, best_b, "(a) wins beyond the spreads" if worst_a < best_b else "NO clear win"), flush=True)

print("(c) the headline render (%%.0f Msamples) on the refitted tree vs a fresh host-SAH tree of the same geometry:" %% (samples / 1e6))
ps = p.copy()
ps.collect_stats = 1
for name, hs in moved.items():
    live.update(hs.desc)
    fresh = api.DeviceScene(hs.desc, 0)
    f_live, f_fresh = live.render(hs.camera, p), fresh.render(hs.camera, p)    # untimed
    same = bool((f_live.view(np.uint64) == f_fresh.view(np.uint64)).all())
    t_live, t_fresh = [], []
    for rep in range(runs):
        for sc, out in ((live, t_live), (fresh, t_fresh)):
            t = time.perf_counter()
            sc.render(hs.camera, p)
            out.append(1e3 * (time.perf_counter() - t))
    visits = []
    for sc in (live, fresh):
        sc.render(hs.camera, ps)
        st = sc.stats()
        visits.append(st.node_visits / max(st.mesh_rays, 1))
    fresh.close()
    t_live, t_fresh = np.array(t_live), np.array(t_fresh)
    print("  displacement %%s: refitted %%.1f ms (min %%.1f, max %%.1f) = %%.0f Msamples/s, %%.2f node visits per mesh ray | fresh %%.1f ms (min %%.1f, max %%.1f) = "
          "%%.0f Msamples/s, %%.2f node visits per mesh ray | refitted / fresh = %%.3f | frames equal bit for bit: %%s"
          %% (name, np.median(t_live), t_live.min(), t_live.max(), samples / np.median(t_live) / 1e3, visits[0], np.median(t_fresh), t_fresh.min(),
             t_fresh.max(), samples / np.median(t_fresh) / 1e3, visits[1], np.median(t_live) / np.median(t_fresh), same), flush=True)
    live.update(base.desc)
live.close()
cold.close()
''' % (REPO,)

runs = 7
for a in sys.argv[1:]:
    if a.startswith("--runs="):
        runs = max(7, int(a.split("=", 1)[1]))
r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", CODE, str(runs)], capture_output=True, text=True)
sys.stdout.write(r.stdout)
if r.returncode != 0:
    sys.stdout.write(r.stderr[-3000:])
    print(f"exit status {r.returncode}: stopping")
    sys.exit(1)
