"""What point queries cost (rt_closest_points).

One process, device-pointer variant, times = the HIP-event time of the query's kernel (rt_point_query_stats), rates in Mpoints/s,
f64 and f32, with the mean BVH nodes visited and triangle tests per point from the counting variant (rt_debug_closest_points_counts):
  * scenes/cornell_dragon (bench.py's mesh): (a) a 128^3 lattice over the box of the frame's first hits, (b) the first hits of a
    1200 x 1200 frame pushed 1e-3 of the scene's extent off the surface along the hit normal;
  * the default scene (no scene file: 455 spheres, walked linearly by every point, and Suzanne): the lattice only.
Beside them rt_trace_rays' kernel_ms for the same number of camera rays (the frame's rays, repeated up to the count), as a
yardstick.  Every side runs once untimed, then `steps` times; median (min, max).  The report goes to stdout and, as Markdown, to
--out (default profiles/closest_points/README.md).  No pass / fail threshold: there is no parent to compare with.

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_closest_points_cost.py [--steps=N] [--out=FILE]   (N >= 3 timed steps per side, default 5)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r)
import torch
import bench
from rust_raytracer_amd import api
steps = int(sys.argv[1])
v = lambda a: np.array(list(a))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
rows = []

def camera_rays(hs):
    cam, W, H = hs.camera, hs.width, hs.height
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = (v(cam.first_pixel) + x[..., None] * v(cam.pixel_delta_u) + y[..., None] * v(cam.pixel_delta_v) - v(cam.position)).reshape(-1, 3)
    return np.broadcast_to(v(cam.position), d.shape).copy(), d

def timed(fn):
    ms = []
    for rep in range(steps + 1):
        t = fn()
        if rep:
            ms.append(t)
    a = np.array(ms)
    return float(np.median(a)), float(a.min()), float(a.max())

def measure(label, sc, pts, cam_o, cam_d):
    n = len(pts)
    d_p = dev(pts)
    d_out = torch.empty(n * 80, dtype=torch.uint8, device="cuda")
    reps = -(-n // len(cam_o))
    d_o, d_d = dev(np.tile(cam_o, (reps, 1))[:n]), dev(np.tile(cam_d, (reps, 1))[:n])
    d_hits = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for prec, pname in ((api.RT_PRECISION_F64, "f64"), (api.RT_PRECISION_F32, "f32")):
        def pq():
            sc.closest_points_device(n, d_p.data_ptr(), d_out.data_ptr(), 0, prec)
            return sc.point_query_stats().kernel_ms
        def rq():
            sc.trace_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr(), prec)
            return sc.ray_query_stats().kernel_ms
        med, lo, hi = timed(pq)
        rmed, rlo, rhi = timed(rq)
        counts = sc.closest_points_counts(pts, precision=prec)
        found = float((d_out.cpu().numpy().view(api.RtPointHit)["flags"] & 1).mean())
        row = (label, pname, n, med, lo, hi, n / med / 1e3, float(counts[:, 0].mean()), float(counts[:, 1].mean()), rmed, rlo, rhi, found)
        rows.append(row)
        print("%%-44s %%s %%9d points  median %%9.3f ms (min %%.3f, max %%.3f) = %%8.1f Mpoints/s  nodes %%7.2f  triangle tests %%7.2f | "
              "rt_trace_rays, as many camera rays: %%9.3f ms (min %%.3f, max %%.3f); found %%.3f" %% row, flush=True)

def lattice(lo, hi, m=128):
    ax = [np.linspace(lo[k], hi[k], m) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)

def first_hits(sc, hs):
    o, d = camera_rays(hs)
    hits = sc.trace_rays(o, d)
    surf = ((hits["flags"] & api.RT_RAY_HIT) != 0) & ((hits["flags"] & api.RT_RAY_ENVIRONMENT) == 0)
    return o, d, hits[surf]

hs = api.HostScene([bench.ensure_dragon(), "-w=1200", "-s=1"])
sc = api.DeviceScene(hs.desc, 0)
o, d, h = first_hits(sc, hs)
P = h["pos"]
extent = float(np.abs(P).max())
print("scenes/cornell_dragon: %%d first hits of a %%dx%%d frame, extent %%.1f; %%d timed steps per side after one untimed" %% (len(P), hs.width, hs.height, extent, steps), flush=True)
measure("cornell_dragon, 128^3 lattice", sc, lattice(P.min(0), P.max(0)), o, d)
measure("cornell_dragon, first hits + 1e-3 extent", sc, np.ascontiguousarray(P + h["normal"] * (1e-3 * extent)), o, d)
sc.close()
hs = api.HostScene(["-w=1200", "-s=1"])
sc = api.DeviceScene(hs.desc, 0)
o, d, h = first_hits(sc, hs)
P = h["pos"][np.isfinite(h["pos"]).all(axis=1)]
P = P[np.abs(P).max(axis=1) < 1e3]   # the ground is one huge sphere: the lattice covers the field of small ones
print("default scene: %%d first hits, lattice over their box" %% len(P), flush=True)
try:
    measure("default scene (455 spheres), 128^3 lattice", sc, lattice(P.min(0), P.max(0)), o, d)
except api.RtError as e:   # a refusal (DESIGN.md section 20) is a result too
    print("default scene: %%s" %% e, flush=True)
sc.close()
with open(sys.argv[2], "w") as f:
    f.write("# Point queries: cost\n\nCommand: `python tools/gpu_closest_points_cost.py --steps=%%d` on one MI355X.  Times are HIP-event times of the "
            "query's kernel (`rt_point_query_stats`), device-pointer variant; every side ran once untimed, then %%d times: median (min, max), which is "
            "the spread of repeated runs.  Nodes and triangle tests per point come from the counting variant (`rt_debug_closest_points_counts`).  "
            "The last columns are `rt_trace_rays_device`'s kernel time for as many camera rays of the same scene (the 1200 x 1200 frame's rays, repeated), "
            "a yardstick and not a comparison of like with like.  Each point of the default scene walks all 455 spheres of the "
            "program, which is the O(primitives) cost of never skipping an `OP_BOUNDS`.  No pass / fail threshold is attached: nothing did this before.\n\n"
            "| points | precision | n | median ms | min | max | Mpoints/s | nodes / point | triangle tests / point | rt_trace_rays ms | min | max | found |\n"
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n" %% (steps, steps))
    for r in rows:
        f.write("| %%s | %%s | %%d | %%.3f | %%.3f | %%.3f | %%.1f | %%.2f | %%.2f | %%.3f | %%.3f | %%.3f | %%.3f |\n" %% r)
''' % (REPO,)

steps, out = 5, os.path.join(REPO, "profiles", "closest_points", "README.md")
for a in sys.argv[1:]:
    if a.startswith("--steps="):
        steps = max(3, int(a.split("=", 1)[1]))
    if a.startswith("--out="):
        out = os.path.abspath(a.split("=", 1)[1])
os.makedirs(os.path.dirname(out), exist_ok=True)
sys.stdout.flush()
r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, "-c", CODE, str(steps), out])   # the child's lines appear as they are printed
if r.returncode != 0:
    print(f"exit status {r.returncode}: stopping")
    sys.exit(1)
