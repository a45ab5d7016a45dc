"""What the fused SH probe bake costs (rt_bake_probes_device).

scenes/cornell_dragon (bench.py's mesh): a grid of G^3 cell-centred probes inside the box (api.probe_grid over 20 .. 535 on every
axis; probes that fall inside the mesh or the box are baked like any other), K = S^2 paths per probe, T = 1, f64.  Two routes
over the same first rays:
  * fused     one call of rt_bake_probes_device: 24 B in and 288 B out per probe;
  * table     what the parent commit can do for the same paths: a table of the same (o, d') - the rays are restated on the host
              in numpy (the generator's SplitMix64, the stratified pair, the uniform sphere; up to the last bits of sine and
              cosine they are the bake's; building them is not timed), uploaded (48 B per path), rendered by
              rt_render_rays_device with S = T = 1 in one call (32 B per path back), downloaded and projected on the host
              (numpy: Y_k(d) * L averaged per probe).  Its paths are keyed by the ray's index in the table, not by (probe,
              stratum): the two routes agree statistically, not bit for bit; band 0 / Y0 averaged over the probes is printed for
              both.  Reported: the whole route, its upload alone, rt_render_rays_device alone (the lower bound of any table
              route), the download + host projection alone, and the kernels-only time of that render (RtRenderStats.kernel_ms).
The share of k_wf_resolve_sh in the fused call is measured with HIP events around the resolve (RT_PROBES_LOG=1 makes the library
print it), against the call's host-clock time.
Every route runs in a child process of its own, once untimed and then `steps` times; median (min, max).  The
report goes to stdout and, as Markdown, is appended to --out (default profiles/bake_probes/cost.md).

Each measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the run.
Usage: python tools/gpu_bake_probes_cost.py [--steps=N] [--grid=G] [--s=S] [--out=FILE]   (N >= 3, default 5; G 32; S 8)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import math, os, re, sys, time
import numpy as np
sys.path.insert(0, %r)
import torch
import bench
from rust_raytracer_amd import api
side, steps, G, S, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
SEED = 7
K = S * S
hs = api.HostScene([bench.ensure_dragon(), "-w=64", "-s=1"])
sc = api.DeviceScene(hs.desc, 0)
pos = api.probe_grid((20.0, 20.0, 20.0), (535.0, 535.0, 535.0), (G, G, G))
n = len(pos)
p = hs.params.copy()
p.sqrt_spt, p.thread_count, p.seed, p.precision = S, 1, SEED, api.RT_PRECISION_F64
p.band_rows, p.n_parts, p.part = 0, 1, 0
p.pipeline, p.collect_stats = api.RT_PIPELINE_AUTO, 0
C0, C1, C2A, C2B, C2C = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396

def clock():
    torch.cuda.synchronize()
    return time.perf_counter()

def med(a):
    a = np.array(a)
    return float(np.median(a)), float(a.min()), float(a.max())

rows = []
def row(name, a):
    m, lo, hi = med(a)
    rows.append("| %%s | %%.3f | %%.3f | %%.3f | %%.1f |" %% (name, m, lo, hi, n * K / m / 1e3))
    print("%%-100s median %%9.3f ms (min %%.3f, max %%.3f) = %%8.1f Mpaths/s" %% (name, m, lo, hi, n * K / m / 1e3), flush=True)

if side == "fused":
    d_pos = torch.from_numpy(pos).cuda()
    d_out = torch.zeros((n, 9, 4), dtype=torch.float64, device="cuda")
    call, kern = [], []
    for rep in range(steps + 1):
        t0 = clock()
        sc.bake_probes_device(n, d_pos.data_ptr(), p, d_out.data_ptr())
        t1 = clock()
        if rep:
            call.append(1e3 * (t1 - t0)); kern.append(sc.stats().kernel_ms)
    row("fused rt_bake_probes_device, %%d^3 probes x %%d paths, f64" %% (G, K), call)
    row("fused, kernels only (RtRenderStats.kernel_ms, resolve included)", kern)
    mean = float((d_out[:, 0, :3] / C0).mean())
    rows.append("| fused: band 0 / Y0 averaged over probes and channels %%.6f | | | | |" %% mean)
    print(rows[-1], flush=True)
else:
    u64 = np.uint64
    def mix(z):
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        return z ^ (z >> u64(31))
    GOLD = u64(0x9E3779B97F4A7C15)
    def build_rays():
        with np.errstate(over="ignore"):
            point = np.repeat(np.arange(n, dtype=np.uint64), K)
            st = np.tile(np.arange(K, dtype=np.uint64), n)
            k = mix(np.full(n * K, (SEED + 0x9E3779B97F4A7C15) %% (1 << 64), dtype=np.uint64))
            k = mix(k ^ (point * u64(0xD1B54A32D192ED03) + u64(0x8CB92BA72F3D8DD7)))
            g = mix(k ^ (st * u64(0xA0761D6478BD642F) + u64(0xE7037ED1A0B428DB)))
            g = g + GOLD; r1 = (mix(g) >> u64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
            g = g + GOLD; r2 = (mix(g) >> u64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        u1 = ((st %% u64(S)).astype(np.float64) + r1) * (1.0 / S)
        u2 = ((st // u64(S)).astype(np.float64) + r2) * (1.0 / S)
        z = 1.0 - 2.0 * u2
        r = np.sqrt(1.0 - z * z)
        phi = u1 * 2.0 * math.pi
        d = np.stack([np.cos(phi) * r, np.sin(phi) * r, z], axis=1)
        o = np.repeat(pos, K, axis=0)
        return np.ascontiguousarray(o), np.ascontiguousarray((o + d) - o), d
    def project(d, L):
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        Y = np.stack([np.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2A * (x * y), C2A * (y * z), C2B * (3.0 * (z * z) - 1.0), C2A * (x * z), C2C * (x * x - y * y)], axis=1)
        return (Y[:, :, None] * L[:, None, :3]).reshape(n, K, 9, 3).mean(axis=1)
    o, d1, d = build_rays()   # the table's construction is not timed: a caller may have the rays already
    p1 = p.copy()
    p1.sqrt_spt = 1
    d_rad = torch.zeros((n * K, 4), dtype=torch.float64, device="cuda")
    whole, up, ren, down, kern = [], [], [], [], []
    for rep in range(steps + 1):
        t0 = clock()
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d1).cuda()
        t1 = clock()
        sc.render_rays_device(n * K, d_o.data_ptr(), d_d.data_ptr(), p1, d_rad.data_ptr())
        t2 = clock()
        sh = project(d, d_rad.cpu().numpy())
        t3 = clock()
        if rep:
            whole.append(1e3 * (t3 - t0)); up.append(1e3 * (t1 - t0)); ren.append(1e3 * (t2 - t1)); down.append(1e3 * (t3 - t2)); kern.append(sc.stats().kernel_ms)
    row("table route: upload, rt_render_rays_device, download + host projection, %%d^3 probes x %%d paths, f64" %% (G, K), whole)
    row("table route, upload alone (48 B per path)", up)
    row("table route, rt_render_rays_device alone (the lower bound of any table route)", ren)
    row("table route, kernels only of that render (RtRenderStats.kernel_ms)", kern)
    row("table route, download (32 B per path) + numpy projection alone", down)
    rows.append("| table route: band 0 / Y0 averaged over probes and channels %%.6f (other streams: statistical agreement only) | | | | |" %% float((sh[:, 0, :] / C0).mean()))
    print(rows[-1], flush=True)
with open(out, "a") as f:
    f.write("\n".join(rows) + "\n")
''' % (REPO,)

steps, grid, s, out = 5, 32, 8, os.path.join(REPO, "profiles", "bake_probes", "cost.md")
for a in sys.argv[1:]:
    if a.startswith("--steps="):
        steps = max(3, int(a.split("=", 1)[1]))
    if a.startswith("--grid="):
        grid = max(1, int(a.split("=", 1)[1]))
    if a.startswith("--s="):
        s = max(1, int(a.split("=", 1)[1]))
    if a.startswith("--out="):
        out = os.path.abspath(a.split("=", 1)[1])
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(f"# SH probe bake: cost on scenes/cornell_dragon\n\nCommand: `python tools/gpu_bake_probes_cost.py --steps={steps} --grid={grid} --s={s}` on one MI355X.  "
            f"{grid}^3 = {grid ** 3} probes (api.probe_grid over 20 .. 535 on every axis), {s * s} paths per probe, T = 1, f64.  Every route in a process of its "
            "own, once untimed and then timed: median (min, max) of host-clock times around work that ends in a device synchronise.\n\n"
            "| side | median ms | min | max | Mpaths/s |\n|---|---|---|---|---|\n")
for side in ("fused", "table"):
    env = dict(os.environ, RT_PROBES_LOG="1" if side == "fused" else "0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", CODE, side, str(steps), str(grid), str(s), out], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stdout.write(r.stderr[-3000:])
        print(f"exit status {r.returncode}: stopping")
        sys.exit(1)
    logs = [ln for ln in r.stderr.splitlines() if ln.startswith("[probes]")]
    if logs:   # the last call's line: resolve kernel time against the call's kernels
        print(logs[-1])
        with open(out, "a") as f:
            f.write(f"| fused, last call: {logs[-1][len('[probes] '):]} | | | | |\n")
