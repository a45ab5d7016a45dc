"""What the fused irradiance bake costs (rt_bake_irradiance_hits_device).

scenes/cornell_dragon (bench.py's mesh) in one process: the points are the first hits of the pixel-centre rays of a 1200 x 1200
frame that lie on a surface (records without a surface point are left out, so that both routes trace the same finite paths),
K = S^2 paths per point (T = 1), S = 4 and 8 in f64, S = 8 in f32.  Two routes over the same points, alternating:
  * fused     one call of rt_bake_irradiance_hits_device on the hit records;
  * unfused   what a caller had to do before, per chunk of 2^22 / K points: a generation step writes the K first rays of every
              point to HBM (eager torch on the device: the generator's SplitMix64 in int64 arithmetic, the stratified
              cosine-weighted direction and the basis of the normal, so the rays are the bake's up to the last bits of sine and
              cosine; 48 B per path), rt_render_rays_device renders them with S = T = 1 (32 B per path back), and a reduction
              averages per point.  Its paths are keyed by the ray's index in the table, not by (point, stratum), so the two
              routes agree statistically, not bit for bit: the means over the surface points are printed side by side.
              Its three parts are also reported on their own: eager torch generation is an upper bound for a caller with a
              generation kernel of their own, rt_render_rays_device alone is the lower bound of any unfused route.
Times are host-clock times around work that ends in a device synchronise.  Every side runs once untimed, then `steps` times in
turn with the other; median (min, max) per side and Mpaths/s.  The report goes to stdout and, as Markdown, to --out (default
profiles/bake_irradiance/README.md).

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_bake_irradiance_cost.py [--steps=N] [--out=FILE]   (N >= 3 timed steps per side, default 5)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import math, os, sys, time
import numpy as np
sys.path.insert(0, %r)
import torch
import bench
from rust_raytracer_amd import api
steps = int(sys.argv[1])
SEED, RAYS = 7, 1 << 22
hs = api.HostScene([bench.ensure_dragon(), "-w=1200", "-s=1"])
cam, W, H = hs.camera, hs.width, hs.height
sc = api.DeviceScene(hs.desc, 0)
v = lambda a: np.array(list(a))
x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
cam_d = (v(cam.first_pixel) + x[..., None] * v(cam.pixel_delta_u) + y[..., None] * v(cam.pixel_delta_v) - v(cam.position)).reshape(-1, 3)
cam_o = np.broadcast_to(v(cam.position), cam_d.shape).copy()
n_px = len(cam_o)
d_o, d_d = torch.from_numpy(cam_o).cuda(), torch.from_numpy(np.ascontiguousarray(cam_d)).cuda()
d_all = torch.zeros(n_px * 96, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
sc.trace_rays_device(n_px, d_o.data_ptr(), d_d.data_ptr(), d_all.data_ptr())
flags = d_all.view(torch.int32).view(n_px, 24)[:, 21]
on_surface = ((flags & 1) != 0) & ((flags & 4) == 0)
# BOTH routes get the records with a surface point and nothing else, so that they trace the same number of paths: a miss
# record has a zero normal, whose non-finite first rays end at their first search and would count as paths all the same
d_hits = d_all.view(n_px, 96)[on_surface].contiguous()
n = int(d_hits.shape[0])
d_out = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
rec = d_hits.view(torch.float64).view(n, 12)
pos, nrm = rec[:, 1:4].contiguous(), rec[:, 4:7].contiguous()
torch.cuda.synchronize()
print("scenes/cornell_dragon %%dx%%d: %%d of %%d pixels see a surface: %%d points for both routes; %%d timed steps per side after one untimed"
      %% (W, H, n, n_px, n, steps), flush=True)

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
    """origins, directions (m * S * S, 3) of points first .. first + m - 1: the bake's first rays"""
    K = S * S
    point = torch.arange(first, first + m, dtype=torch.int64, device="cuda")[:, None].expand(m, K)
    st = torch.arange(K, dtype=torch.int64, device="cuda")[None, :].expand(m, K)
    g = key(SEED, point, st)
    g, r1 = uniform(g)
    g, r2 = uniform(g)
    u1 = ((st %% S).double() + r1) * (1.0 / S)
    u2 = ((st // S).double() + r2) * (1.0 / S)
    phi = u1 * 2.0 * math.pi
    sq = torch.sqrt(u2)
    lx, ly, lz = torch.cos(phi) * sq, torch.sin(phi) * sq, torch.sqrt(1.0 - u2)
    w = nrm[first:first + m]
    w = w / torch.sqrt((w * w).sum(dim=1, keepdim=True))
    a = torch.where((w[:, 0].abs() > 0.9)[:, None], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device="cuda"),
                    torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device="cuda"))
    vv = torch.linalg.cross(w, a)
    vv = vv / torch.sqrt((vv * vv).sum(dim=1, keepdim=True))
    uu = torch.linalg.cross(w, vv)
    d = uu[:, None, :] * lx[..., None] + vv[:, None, :] * ly[..., None] + w[:, None, :] * lz[..., None]
    o = pos[first:first + m][:, None, :].expand(m, K, 3)
    return o.reshape(-1, 3).contiguous(), ((o + d) - o).reshape(-1, 3).contiguous()

def params(S, prec):
    p = hs.params.copy()
    p.sqrt_spt, p.thread_count, p.seed, p.precision = S, 1, SEED, prec
    p.band_rows, p.n_parts, p.part = 0, 1, 0
    p.pipeline, p.collect_stats = api.RT_PIPELINE_AUTO, 0
    return p

def clock():
    torch.cuda.synchronize()
    return time.perf_counter()

means = {}
parts = {}   # of the last unfused run: generation, render, reduction (ms)
d_rad = torch.zeros((RAYS, 4), dtype=torch.float64, device="cuda")
def unfused(S, prec):
    K = S * S
    chunk = RAYS // K
    p1 = params(1, prec)
    res = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    gen = ren = red = 0.0
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        t0 = clock(); o, d = generate(first, m, S)
        t1 = clock(); sc.render_rays_device(m * K, o.data_ptr(), d.data_ptr(), p1, d_rad.data_ptr())
        t2 = clock(); res[first:first + m] = d_rad[: m * K].view(m, K, 4).sum(dim=1) / K
        t3 = clock()
        gen += t1 - t0; ren += t2 - t1; red += t3 - t2
    means["unfused"] = float(res[:, :3].mean())
    parts["generate"], parts["render"], parts["reduce"] = 1e3 * gen, 1e3 * ren, 1e3 * red
    return 1e3 * (gen + ren + red)
def fused(S, prec):
    p = params(S, prec)
    t0 = clock()
    sc.bake_irradiance_hits_device(n, d_hits.data_ptr(), p, d_out.data_ptr())
    t1 = clock()
    means["fused"] = float(d_out[:, :3].mean())
    return 1e3 * (t1 - t0)

report = []
for prec, pname, S in ((api.RT_PRECISION_F64, "f64", 4), (api.RT_PRECISION_F64, "f64", 8), (api.RT_PRECISION_F32, "f32", 8)):
    K = S * S
    sides = [("fused bake, %%d paths per point, %%s" %% (K, pname), lambda: fused(S, prec)),
             ("unfused: generate, rt_render_rays_device, reduce, %%d paths per point, %%s" %% (K, pname), lambda: unfused(S, prec))]
    rows = {name: [] for name, _ in sides}
    part_names = (("generate", "unfused, generation alone (eager torch: an upper bound for a caller's own kernel)"),
                  ("render", "unfused, rt_render_rays_device alone (the lower bound of the unfused route)"), ("reduce", "unfused, reduction alone"))
    for _, label in part_names:
        rows["%%s, %%d paths per point, %%s" %% (label, K, pname)] = []
    for rep in range(steps + 1):
        for name, fn in sides:
            ms = fn()
            if rep:
                rows[name].append(ms)
        if rep:
            for k, label in part_names:
                rows["%%s, %%d paths per point, %%s" %% (label, K, pname)].append(parts[k])
    for name in rows:
        a = np.array(rows[name])
        med = float(np.median(a))
        report.append((name, med, float(a.min()), float(a.max()), n * K / med / 1e3))
        print("%%-110s median %%9.3f ms (min %%.3f, max %%.3f) = %%8.1f Mpaths/s" %% report[-1], flush=True)
    line = "%%d paths per point, %%s: mean over the surface points of (r + g + b) / 3: fused %%.6f, unfused %%.6f (other streams: statistical agreement only)" %% (K, pname, means["fused"], means["unfused"])
    print(line, flush=True)
    report.append((line,))
with open(sys.argv[2], "w") as f:
    f.write("# Irradiance bake: cost on scenes/cornell_dragon\n\nCommand: `python tools/gpu_bake_irradiance_cost.py --steps=%%d` on one MI355X.  %%d points = the first hits of a "
            "%%dx%%d frame that lie on a surface (%%.1f %%%% of its pixels; the records without a surface point are left out for BOTH routes, so both trace the same number of finite paths).  "
            "Fused: one `rt_bake_irradiance_hits_device` call.  Unfused: per chunk of 2^22 paths, generation of the first rays by eager torch on the device + "
            "`rt_render_rays_device` with S = T = 1 + the reduction; the three parts are also listed on their own, because the generation is dozens of elementwise torch kernels "
            "with n x K x 3 temporaries and says little about a caller with a generation kernel of their own: the honest comparison is the fused bake against "
            "`rt_render_rays_device` alone, which no unfused route can beat.  Host-clock times around work that ends in a device synchronise.  Every side ran once untimed, "
            "then %%d times in turn with the other: median (min, max), which is the spread of repeated runs.\n\n"
            "| side | median ms | min | max | Mpaths/s |\n|---|---|---|---|---|\n" %% (steps, n, W, H, 100.0 * n / n_px, steps))
    for row in report:
        if len(row) == 1:
            f.write("| %%s | | | | |\n" %% row[0])
        else:
            f.write("| %%s | %%.3f | %%.3f | %%.3f | %%.1f |\n" %% row)
''' % (REPO,)

steps, out = 5, os.path.join(REPO, "profiles", "bake_irradiance", "README.md")
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
