"""What rasterising a lightmap costs (rt_lightmap_texels_device), next to the bake that follows it.

One process, device-pointer variants.  Per scene and map size: rt_lightmap_stats of the rasterisation (binning = per-tile
counts + scan + fill, and the raster kernel, HIP-event times), the tile references and the covered share, and the kernel time
(rt_get_stats) of rt_bake_irradiance_hits_device at 64 paths per texel (S = 8, T = 1) on the same records, so that a reader
sees what share of a bake the new stage is.  Scenes: scenes/resource/monkey.obj (15 744 triangles) under one transform at
1024^2 and 4096^2, and bench.py's dragon if its mesh carries UVs.  Method: one untimed pair of calls, then `steps` pairs,
rasterisation and bake alternating; median (min, max).  The report is a Markdown table on stdout (profiles/lightmap/README.md
holds one).  No pass / fail threshold: the parent cannot do this at all.

The measurement runs in a child process under `timeout -k 10 <limit>`; a child that times out or dies on a signal ends the
run.  Usage: python tools/gpu_lightmap_cost.py [--steps=N] [--sizes=1024,4096]"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import os, sys, tempfile
import numpy as np
sys.path.insert(0, %r)
import torch
import bench
from rust_raytracer_amd import api
steps = int(sys.argv[1])
sizes = [int(x) for x in sys.argv[2].split(",")]
REPO = %r

def stat3(a):
    a = np.array(a)
    return "%%.3f (%%.3f, %%.3f)" %% (float(np.median(a)), float(a.min()), float(a.max()))

def measure(label, hs, node):
    sc = api.DeviceScene(hs.desc, 0)
    p = type(hs.params).from_buffer_copy(hs.params)
    p.sqrt_spt, p.thread_count, p.pipeline, p.collect_stats = 8, 1, api.RT_PIPELINE_AUTO, 0
    p.band_rows = p.n_parts = p.part = 0
    for w in sizes:
        n = w * w
        d_hits = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
        d_out = torch.empty(n * 4, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        bins, rasters, bakes = [], [], []
        for rep in range(steps + 1):
            sc.lightmap_texels_device(node, w, w, d_hits.data_ptr())
            st = sc.lightmap_stats()
            sc.bake_irradiance_hits_device(n, d_hits.data_ptr(), p, d_out.data_ptr())
            bake_ms = sc.stats().kernel_ms
            if rep:
                bins.append(st.bin_ms); rasters.append(st.raster_ms); bakes.append(bake_ms)
        share = (np.median(bins) + np.median(rasters)) / (np.median(bins) + np.median(rasters) + np.median(bakes))
        print("| %%s | %%d x %%d | %%d | %%.3f | %%s | %%s | %%s | %%.2f %%%% |" %% (label, w, w, st.tile_refs, st.covered_texels / st.texels, stat3(bins), stat3(rasters),
              stat3(bakes), 100.0 * share), flush=True)
        del d_hits, d_out
    sc.close()

print("| scene | map | tile references | covered share | binning ms: median (min, max) | raster ms | rt_bake_irradiance_hits_device, 64 paths, kernel ms | rasterisation's share of the two |")
print("|---|---|---|---|---|---|---|---|", flush=True)
tmp = tempfile.mkdtemp(prefix="lightmap_cost_")
scene = os.path.join(tmp, "monkey")
with open(scene, "w") as f:
    f.write("@config output_width = 64\n@config aspect_ratio = 1\n@config focal_length = 40\n@config camera_pos = 0,1.5,6\n@config camera_target = 0,0.5,0\n"
            "white: lambertian (constant 0.73,0.73,0.73)\nfloor: plane 0,-1,0 5,0,0 0,0,-5 $white\n"
            "m: transform (mesh %%s $white) ry=30 t=0,0.2,0\n"
            "light: plane 0,4,0 1.5,0,0 0,0,1.5 (emissive (constant 10,10,10)) backface\nworld: list $floor $m $light\nlights: list $light\n"
            %% os.path.relpath(os.path.join(REPO, "scenes", "resource", "monkey.obj"), tmp))
def mesh_nodes(hs):
    d = hs.desc.contents
    return [i for i in range(d.n_nodes) if d.nodes[i].type == 3]
hs = api.HostScene([scene, "-w=64", "-s=1", "--seed=7"])
measure("monkey.obj (15 744 triangles)", hs, mesh_nodes(hs)[0])
hs = api.HostScene([bench.ensure_dragon(), "-w=64", "-s=1"])
nodes = mesh_nodes(hs)
d = hs.desc.contents
with_uv = [i for i in nodes if d.meshes[d.nodes[i].mesh].uvs and d.meshes[d.nodes[i].mesh].tri_uv]
if with_uv:
    measure("cornell_dragon (%%d triangles)" %% d.meshes[d.nodes[with_uv[0]].mesh].n_triangles, hs, with_uv[0])
else:
    print("cornell_dragon: its mesh carries no UVs: not measured", flush=True)
'''


def main():
    steps, sizes = 5, "1024,4096"
    for a in sys.argv[1:]:
        if a.startswith("--steps="):
            steps = max(3, int(a.split("=", 1)[1]))
        elif a.startswith("--sizes="):
            sizes = a.split("=", 1)[1]
    r = subprocess.run(["timeout", "-k", "10", "480", sys.executable, "-c", CODE % (REPO, REPO), str(steps), sizes], cwd=REPO)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
