"""What the fused ambient-occlusion bake costs (rt_bake_visibility_hits_device).

scenes/cornell_dragon (bench.py's mesh) in one process: the points are the first hits of the pixel-centre rays of a 1200 x 1200
frame, S = 64 and 256 samples per point, f64 and f32.  Two routes over the same points, alternating:
  * fused     one call of rt_bake_visibility_hits_device on the hit records; time = the HIP-event time of the bake kernel
              (rt_bake_stats);
  * unfused   (its three parts are also reported separately: eager torch generation is an upper bound, the occlusion kernel
              alone the lower bound of any unfused route) what a caller had to do before: per chunk of 2^16 points a generation step writes the S rays of every point to
              HBM (torch on the device: the generator's SplitMix64 in int64 arithmetic, the cosine-weighted direction and the
              basis of the normal, so the rays are the bake's up to the last bits of sine and cosine), rt_occluded_device
              answers them over (bias, max_distance), and a reduction counts per point; time = generation + reduction (torch
              events) + the occlusion kernel (rt_ray_query_stats).
Every side runs once untimed, then `steps` times in turn with the other; median (min, max) per side, points/s and rays/s, and
the share of points on which the two routes count the same.  The report goes to stdout and, as Markdown, to --out (default
profiles/bake/README.md).

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_bake_cost.py [--steps=N] [--out=FILE]   (N >= 3 timed steps per side, default 3)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import math, os, sys
import numpy as np
sys.path.insert(0, %r)
import torch
import bench
from rust_raytracer_amd import api
steps = int(sys.argv[1])
BIAS, SEED, CHUNK = 1e-3, 7, 1 << 16
hs = api.HostScene([bench.ensure_dragon(), "-w=1200", "-s=1"])
cam, W, H = hs.camera, hs.width, hs.height
sc = api.DeviceScene(hs.desc, 0)
v = lambda a: np.array(list(a))
x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
cam_d = (v(cam.first_pixel) + x[..., None] * v(cam.pixel_delta_u) + y[..., None] * v(cam.pixel_delta_v) - v(cam.position)).reshape(-1, 3)
cam_o = np.broadcast_to(v(cam.position), cam_d.shape).copy()
n = len(cam_o)
d_o, d_d = torch.from_numpy(cam_o).cuda(), torch.from_numpy(np.ascontiguousarray(cam_d)).cuda()
d_hits = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
sc.trace_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr())
rec = d_hits.view(torch.float64).view(n, 12)
flags = d_hits.view(torch.int32).view(n, 24)[:, 21]
surface = ((flags & 1) != 0) & ((flags & 4) == 0)
pos, nrm = rec[:, 1:4].contiguous(), rec[:, 4:7].contiguous()
nrm = torch.where(surface[:, None], nrm, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device="cuda"))  # a record without a surface has no normal: finite rays all the same
extent = float(pos[surface].abs().max())
max_distance = 0.25 * extent
print("scenes/cornell_dragon %%dx%%d: %%d points (%%.1f %%%% on a surface), bias %%g, max_distance %%g (a quarter of the extent); %%d timed steps per side after one untimed"
      %% (W, H, n, 100 * float(surface.float().mean()), BIAS, max_distance, steps), flush=True)

def shr(z, k):   # int64 arithmetic wraps like uint64; only the right shifts need the sign bits cleared
    return (z >> k) & ((1 << (64 - k)) - 1)
def i64(c):
    return c - (1 << 64) if c >= (1 << 63) else c
def mix(z):
    z = (z ^ shr(z, 30)) * i64(0xBF58476D1CE4E5B9)
    z = (z ^ shr(z, 27)) * i64(0x94D049BB133111EB)
    return z ^ shr(z, 31)
GOLD = i64(0x9E3779B97F4A7C15)
def key(seed, point, s):   # Rng::key(seed, 0, point, s)
    k = mix(torch.full_like(point, i64((seed + 0x9E3779B97F4A7C15) %% (1 << 64))))
    k = mix(k ^ (point * i64(0xD1B54A32D192ED03) + i64(0x8CB92BA72F3D8DD7)))
    return mix(k ^ (s * i64(0xA0761D6478BD642F) + i64(0xE7037ED1A0B428DB)))
def uniform(state):
    state = state + GOLD
    return state, shr(mix(state), 11).double() * (1.0 / 9007199254740992.0)

def generate(first, m, S):
    """origins, directions (m * S, 3) of points first .. first + m - 1"""
    point = torch.arange(first, first + m, dtype=torch.int64, device="cuda")[:, None].expand(m, S)
    s = torch.arange(S, dtype=torch.int64, device="cuda")[None, :].expand(m, S)
    st = key(SEED, point, s)
    st, r1 = uniform(st)
    st, r2 = uniform(st)
    phi = r1 * 2.0 * math.pi
    sq = torch.sqrt(r2)
    lx, ly, lz = torch.cos(phi) * sq, torch.sin(phi) * sq, torch.sqrt(1.0 - r2)
    w = nrm[first:first + m]
    w = w / torch.sqrt((w * w).sum(dim=1, keepdim=True))
    a = torch.where((w[:, 0].abs() > 0.9)[:, None], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device="cuda"),
                    torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device="cuda"))
    vv = torch.linalg.cross(w, a)
    vv = vv / torch.sqrt((vv * vv).sum(dim=1, keepdim=True))
    uu = torch.linalg.cross(w, vv)
    d = uu[:, None, :] * lx[..., None] + vv[:, None, :] * ly[..., None] + w[:, None, :] * lz[..., None]
    o = pos[first:first + m][:, None, :].expand(m, S, 3)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()

d_occ = torch.zeros(CHUNK * 256, dtype=torch.uint8, device="cuda")
counts = {}
parts = {}   # of the last unfused run: generation, occlusion kernel, reduction (ms)
def unfused(S, prec):
    gen = occ = red = 0.0
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    hi = torch.full((CHUNK * S,), max_distance, dtype=torch.float64, device="cuda")
    lo = torch.full((CHUNK * S,), BIAS, dtype=torch.float64, device="cuda")
    for first in range(0, n, CHUNK):
        m = min(CHUNK, n - first)
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record(); o, d = generate(first, m, S); e1.record(); torch.cuda.synchronize()
        sc.occluded_device(m * S, o.data_ptr(), d.data_ptr(), d_occ.data_ptr(), lo.data_ptr(), hi.data_ptr(), prec)
        ms = sc.ray_query_stats().kernel_ms
        e2.record(); cnt[first:first + m] = S - d_occ[: m * S].view(m, S).sum(dim=1, dtype=torch.int64); e3.record(); torch.cuda.synchronize()
        gen += e0.elapsed_time(e1); occ += ms; red += e2.elapsed_time(e3)
    counts["unfused"] = torch.where(surface, cnt, torch.full_like(cnt, S))
    parts["generate"], parts["occlusion"], parts["reduce"] = gen, occ, red
    return gen + occ + red
def fused(S, prec):
    bp = api.RtBakeParams.defaults(samples=S, seed=SEED, bias=BIAS, max_distance=max_distance, precision=prec)
    sc.bake_visibility_hits_device(n, d_hits.data_ptr(), d_out.data_ptr(), bp)
    counts["fused"] = torch.round(d_out.view(torch.float64).view(n, 4)[:, 0] * S).long()
    return sc.bake_stats().kernel_ms

report = []
for prec, pname in ((api.RT_PRECISION_F64, "f64"), (api.RT_PRECISION_F32, "f32")):
    for S in (64, 256):
        sides = [("fused bake, S = %%d, %%s" %% (S, pname), lambda: fused(S, prec)), ("unfused: generate, rt_occluded_device, reduce, S = %%d, %%s" %% (S, pname), lambda: unfused(S, prec))]
        rows = {name: [] for name, _ in sides}
        part_names = (("generate", "unfused, generation alone (eager torch: an upper bound for a caller's own kernel)"),
                      ("occlusion", "unfused, rt_occluded_device alone (the lower bound of the unfused route)"), ("reduce", "unfused, reduction alone"))
        for _, label in part_names:
            rows["%%s, S = %%d, %%s" %% (label, S, pname)] = []
        for rep in range(steps + 1):
            for name, fn in sides:
                ms = fn()
                if rep:
                    rows[name].append(ms)
            if rep:
                for k, label in part_names:
                    rows["%%s, S = %%d, %%s" %% (label, S, pname)].append(parts[k])
        for name in rows:
            a = np.array(rows[name])
            med = float(np.median(a))
            report.append((name, med, float(a.min()), float(a.max()), n / med / 1e3, n * S / med / 1e3))
            print("%%-100s median %%9.3f ms (min %%.3f, max %%.3f) = %%7.2f Mpoints/s, %%8.1f Mrays/s" %% report[-1], flush=True)
        same = float((counts["fused"] == counts["unfused"]).float().mean())
        vis = float(counts["fused"][surface].double().mean()) / S
        line = "S = %%d, %%s: the two routes count the same on %%.4f %%%% of the points; mean visibility on surfaces %%.4f" %% (S, pname, 100 * same, vis)
        print(line, flush=True)
        report.append((line,))
with open(sys.argv[2], "w") as f:
    f.write("# Ambient-occlusion bake: cost on scenes/cornell_dragon\n\nCommand: `python tools/gpu_bake_cost.py --steps=%%d` on one MI355X.  %%d points = the first hits of a "
            "%%dx%%d frame (%%.1f %%%% on a surface; the others are skipped by the fused route and masked out of the unfused one, which still traces their rays), bias %%g, max_distance %%g.  "
            "Fused: HIP-event time of the bake kernel (`rt_bake_stats`).  Unfused: per chunk of 2^16 points, generation of the rays by eager torch on the device + the occlusion kernel "
            "(`rt_ray_query_stats`) + the reduction; the three parts are also listed on their own, because the generation is dozens of elementwise torch kernels with n x S x 3 "
            "temporaries and says little about a caller with a generation kernel of their own: the honest comparison is the fused bake against `rt_occluded_device` alone, "
            "which no unfused route can beat.  Every side ran once untimed, then %%d times in turn with the other: median (min, max), which is the spread of repeated runs.\n\n"
            "| side | median ms | min | max | Mpoints/s | Mrays/s |\n|---|---|---|---|---|---|\n" %% (steps, n, W, H, 100 * float(surface.float().mean()), BIAS, max_distance, steps))
    for row in report:
        if len(row) == 1:
            f.write("| %%s | | | | | |\n" %% row[0])
        else:
            f.write("| %%s | %%.3f | %%.3f | %%.3f | %%.2f | %%.1f |\n" %% row)
''' % (REPO,)

steps, out = 3, os.path.join(REPO, "profiles", "bake", "README.md")
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
