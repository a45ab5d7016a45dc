"""Builds the native libraries in-tree (the built .so files travel to the GPU box with the
repo snapshot).  hipcc cross-compiles for gfx950 without a GPU.

    python -m rust_raytracer_amd.build            # everything
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
HOST_SRC = ["scene_builder.cpp", "obj_loader.cpp", "config.cpp", "dsl_loader.cpp", "default_scene.cpp",
            "output.cpp", "host_api.cpp", "image_loader.cpp"]
DEVICE_SRC = ["rt_kernels.hip", "rt_accum.hip", "rt_aov.hip", "rt_query.hip", "rt_bake.hip", "rt_point.hip", "rt_lightmap.hip", "rt_bvh_device.hip", "rt_refit.hip", "rt_compile.cpp", "rt_bvh.cpp", "rt_tables.cpp", "rt_desc.cpp"]
DEVICE_HDR = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))  # every header: a stale library can never be what the tests run


def _digest(sources, extra="") -> str:
    h = hashlib.sha256(extra.encode())
    for s in sources:
        h.update(os.path.basename(s).encode())
        with open(s, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _newer(target: str, sources, extra="") -> bool:
    """True when `target` must be (re)built: it is missing, or the CONTENT of its sources (and the
    flags in `extra`) differs from what it was built from (digest kept beside it in `<target>.srchash`;
    file times are not trusted: a snapshot copied to the GPU box does not keep them)."""
    if not os.path.exists(target):
        return True
    try:
        with open(target + ".srchash") as f:
            return f.read().strip() != _digest(sources, extra)
    except OSError:
        return True


def _stamp(target: str, sources, extra="") -> None:
    with open(target + ".srchash", "w") as f:
        f.write(_digest(sources, extra) + "\n")


def _run(cmd, cwd=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"command failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return r


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def build_host(force: bool = False) -> str:
    out = os.path.join(PKG_DIR, "librt_host.so")
    hdir = os.path.join(CSRC, "host")
    srcs = [os.path.join(hdir, s) for s in HOST_SRC]
    deps = srcs + [os.path.join(hdir, h) for h in ("hmath.h", "scene_builder.h", "host_internal.h")] + \
        [os.path.join(REPO_DIR, "include", h) for h in ("rt_mi355.h", "rt_host.h", "rt_detmath.h")]
    if force or _newer(out, deps):
        # -ffp-contract=off: rth_probe_rays promises one rounding per operation, whatever the target's instruction set
        _run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra", "-o", out] + srcs + ["-lz"])
        _stamp(out, deps)
    return out


def build_cli(force: bool = False) -> str:
    """The `rtrace` executable: drop-in for the reference binary (same flags, DSL, out.png)."""
    out = os.path.join(PKG_DIR, "rtrace")
    src = os.path.join(CSRC, "host", "main.cpp")
    if not os.path.exists(src):
        return ""
    deps = [src] + [os.path.join(REPO_DIR, "include", h) for h in ("rt_mi355.h", "rt_host.h")]
    if force or _newer(out, deps):
        _run([hipcc_path(), "-std=c++17", "-O2", "-o", out, src, "-L" + PKG_DIR, "-lrt_host", "-lrt_mi355",
              "-Wl,-rpath,$ORIGIN", "-lpthread"])
        _stamp(out, deps)
    return out


def build_device(force: bool = False) -> str:
    out = os.path.join(PKG_DIR, "librt_mi355.so")
    srcs = [os.path.join(CSRC, s) for s in DEVICE_SRC]
    deps = srcs + [os.path.join(CSRC, h) for h in DEVICE_HDR] + \
        [os.path.join(REPO_DIR, "include", h) for h in ("rt_mi355.h", "rt_detmath.h")]
    extra = os.environ.get("RT_EXTRA_HIPCC_FLAGS", "").split()
    if force or _newer(out, deps, " ".join(extra)):
        # -ffp-contract=off: the reference is Rust, which never fuses a*b+c; with the deterministic
        # sin/cos/log of include/rt_detmath.h the f64 kernels then follow the oracle's paths bit for
        # bit.  Measured cost on the headline scene: 3 % (the kernel is latency-bound, not FMA-bound).
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
              "-Wall", "-Wno-unused-function"] + extra + ["-o", out] + srcs)
        _stamp(out, deps, " ".join(extra))
    return out


def build_oracle(force: bool = False) -> str:
    odir = os.path.join(REPO_DIR, "oracle")
    out = os.path.join(odir, "liboracle.so")
    deps = [os.path.join(odir, "oracle.cpp"), os.path.join(odir, "oracle.h"),
            os.path.join(REPO_DIR, "include", "rt_mi355.h"), os.path.join(REPO_DIR, "include", "rt_detmath.h")]
    if force or _newer(out, deps):
        _run(["make", "-C", odir, "-B", "liboracle.so"])
        _stamp(out, deps)
    return out


def build_tools(force: bool = False) -> str:
    out = os.path.join(REPO_DIR, "tools", "gen_dragon")
    src = os.path.join(REPO_DIR, "tools", "gen_dragon.cpp")
    if os.path.exists(src) and (force or _newer(out, [src])):
        _run(["g++", "-std=c++17", "-O2", "-o", out, src])
        _stamp(out, [src])
    # micro-benchmark that pins the traversal kernel's roofline (random-line gather rates)
    ub_src = os.path.join(REPO_DIR, "tools", "ubench", "gather_lines.hip")
    ub_out = os.path.join(REPO_DIR, "tools", "ubench", "gather_lines")
    if os.path.exists(ub_src) and (force or _newer(ub_out, [ub_src])):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-o", ub_out, ub_src])
        _stamp(ub_out, [ub_src])
    return out


def build_all(force: bool = False):
    return {"host": build_host(force), "device": build_device(force), "cli": build_cli(force),
            "oracle": build_oracle(force), "tools": build_tools(force)}


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv))
