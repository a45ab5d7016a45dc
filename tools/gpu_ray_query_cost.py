"""What ray queries cost (rt_trace_rays / rt_occluded).

scenes/cornell_dragon (bench.py's mesh) in one process, device-pointer variants, times = the HIP-event time of the query's
kernels (rt_ray_query_stats), rates in Mrays/s:
  * closest hit and occlusion for the camera rays of a 1200 x 1200 frame (pixel centres: coherent) and for their follow-up
    rays (from the hit points into random directions: incoherent), f64 and f32;
  * on the segments between permuted hit points: the any-hit kernel against "closest hit, then t < t_max", alternating;
  * RT_RQ_CHUNK from 2^20 to 2^24 on the camera rays repeated 12 times (17.3 M rays), closest hit, f64.
Every side runs once untimed, then `steps` times in turn with the others; median (min, max) per side.  The report goes to
stdout and, as Markdown, to --out (default profiles/ray_queries/README.md).

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_ray_query_cost.py [--steps=N] [--out=FILE]   (N >= 3 timed steps per side, default 5)"""
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
hs = api.HostScene([bench.ensure_dragon(), "-w=1200", "-s=1"])
cam, W, H = hs.camera, hs.width, hs.height
sc = api.DeviceScene(hs.desc, 0)
v = lambda a: np.array(list(a))
x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
cam_d = (v(cam.first_pixel) + x[..., None] * v(cam.pixel_delta_u) + y[..., None] * v(cam.pixel_delta_v) - v(cam.position)).reshape(-1, 3)
cam_o = np.broadcast_to(v(cam.position), cam_d.shape).copy()
hits = sc.trace_rays(cam_o, cam_d)
surf = ((hits["flags"] & api.RT_RAY_HIT) != 0) & ((hits["flags"] & api.RT_RAY_ENVIRONMENT) == 0)
P = np.ascontiguousarray(hits["pos"][surf])
rng = np.random.default_rng(31)
fu_d = rng.normal(size=P.shape)
fu_d *= (rng.uniform(0.5, 2, size=len(P)) / np.linalg.norm(fu_d, axis=1))[:, None]
seg_d = P[rng.permutation(len(P))] - P
print("scenes/cornell_dragon %%dx%%d: %%d camera rays (%%.1f %%%% hit a surface), %%d follow-up rays, %%d segments; %%d timed steps per side after one untimed"
      %% (W, H, len(cam_o), 100 * surf.mean(), len(P), len(P), steps), flush=True)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
sets = {"camera": (dev(cam_o), dev(cam_d)), "follow-up": (dev(P), dev(fu_d)), "segments": (dev(P), dev(seg_d))}
n_max = 12 * len(cam_o)
d_hits = torch.empty(n_max * 96, dtype=torch.uint8, device="cuda")
d_occ = torch.empty(n_max, dtype=torch.uint8, device="cuda")
d_lo = torch.full((len(P),), 1e-3, dtype=torch.float64, device="cuda")
d_hi = torch.full((len(P),), 0.999, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()

def closest(o, d, prec):
    sc.trace_rays_device(len(o), o.data_ptr(), d.data_ptr(), d_hits.data_ptr(), prec)
    return sc.ray_query_stats().kernel_ms
def occl(o, d, prec, lo=0, hi=0):
    sc.occluded_device(len(o), o.data_ptr(), d.data_ptr(), d_occ.data_ptr(), lo, hi, prec)
    return sc.ray_query_stats().kernel_ms
def closest_then_compare(o, d, prec):
    ms = closest(o, d, prec)
    t = d_hits[: len(o) * 96].view(torch.float64).view(-1, 12)[:, 0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); occ = t < 0.999; e1.record(); torch.cuda.synchronize()
    closest_then_compare.last = occ
    return ms + e0.elapsed_time(e1)

def run(sides):
    rows = {name: [] for name, _, _ in sides}
    for rep in range(steps + 1):
        for name, n, fn in sides:
            ms = fn()
            if rep:
                rows[name].append(ms)
    out = []
    for name, n, _ in sides:
        a = np.array(rows[name])
        out.append((name, n, float(np.median(a)), float(a.min()), float(a.max())))
        print("%%-58s %%9d rays  median %%8.3f ms (min %%.3f, max %%.3f) = %%8.1f Mrays/s" %% (name, n, out[-1][2], out[-1][3], out[-1][4], n / out[-1][2] / 1e3), flush=True)
    return out

report = []
for prec, pname in ((api.RT_PRECISION_F64, "f64"), (api.RT_PRECISION_F32, "f32")):
    sides = []
    for sname in ("camera", "follow-up"):
        o, d = sets[sname]
        sides.append(("closest hit, %%s rays, %%s" %% (sname, pname), len(o), lambda o=o, d=d: closest(o, d, prec)))
        sides.append(("occlusion (0.001, inf), %%s rays, %%s" %% (sname, pname), len(o), lambda o=o, d=d: occl(o, d, prec)))
    o, d = sets["segments"]
    sides.append(("segments: any-hit kernel, %%s" %% pname, len(o), lambda o=o, d=d: occl(o, d, prec, d_lo.data_ptr(), d_hi.data_ptr())))
    sides.append(("segments: closest hit, then t < t_max, %%s" %% pname, len(o), lambda o=o, d=d: closest_then_compare(o, d, prec)))
    report += run(sides)
    occl(o, d, prec, d_lo.data_ptr(), d_hi.data_ptr())
    closest_then_compare(o, d, prec)
    same = bool(torch.equal(d_occ[: len(o)].bool(), closest_then_compare.last))
    print("segments, %%s: the two ways agree on every segment: %%s (%%.1f %%%% occluded)" %% (pname, same, 100 * float(d_occ[: len(o)].float().mean())), flush=True)
    report.append(("segments, %%s: the two ways agree on every segment: %%s" %% (pname, same), 0, 0.0, 0.0, 0.0))

big_o, big_d = sets["camera"][0].repeat(12, 1), sets["camera"][1].repeat(12, 1)
sides = []
for sh in (20, 21, 22, 23, 24):
    def fn(sh=sh):
        os.environ["RT_RQ_CHUNK"] = str(1 << sh)
        return closest(big_o, big_d, api.RT_PRECISION_F64)
    sides.append(("closest hit, camera rays x 12, f64, RT_RQ_CHUNK = 2^%%d" %% sh, len(big_o), fn))
report += run(sides)
with open(sys.argv[2], "w") as f:
    f.write("# Ray queries: cost on scenes/cornell_dragon\n\nCommand: `python tools/gpu_ray_query_cost.py --steps=%%d` on one MI355X.  Times are HIP-event times of the "
            "query's kernels (`rt_ray_query_stats`), device-pointer variants; every side ran once untimed, then %%d times in turn with the others "
            "of its table: median (min, max), which is the spread of repeated runs.  %%d camera rays (%%.1f %%%% hit a surface), %%d follow-up rays and segments.\n\n"
            "| side | rays | median ms | min | max | Mrays/s |\n|---|---|---|---|---|---|\n" %% (steps, steps, len(cam_o), 100 * surf.mean(), len(P)))
    for name, n, med, lo, hi in report:
        if n:
            f.write("| %%s | %%d | %%.3f | %%.3f | %%.3f | %%.1f |\n" %% (name, n, med, lo, hi, n / med / 1e3))
        else:
            f.write("| %%s | | | | | |\n" %% name)
''' % (REPO,)

steps, out = 5, os.path.join(REPO, "profiles", "ray_queries", "README.md")
for a in sys.argv[1:]:
    if a.startswith("--steps="):
        steps = max(3, int(a.split("=", 1)[1]))
    if a.startswith("--out="):
        out = os.path.abspath(a.split("=", 1)[1])
os.makedirs(os.path.dirname(out), exist_ok=True)
r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", CODE, str(steps), out], capture_output=True, text=True)
sys.stdout.write(r.stdout)
if r.returncode != 0:
    sys.stdout.write(r.stderr[-3000:])
    print(f"exit status {r.returncode}: stopping")
    sys.exit(1)
