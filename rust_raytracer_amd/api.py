"""ctypes mirror of include/rt_mi355.h and include/rt_host.h.

The product path is `librt_mi355.so` (HIP kernels behind the C ABI) plus `librt_host.so`
(CLI flags, scene DSL, OBJ loader, camera, output stage).  There is NO CPU fallback: if the
HIP library is missing, `load_device_lib()` raises.  The CPU oracle under oracle/ is test
infrastructure and is never loaded from this package.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional, Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)

RT_OK = 0
RT_E_INVALID, RT_E_UNSUPPORTED, RT_E_DEVICE, RT_E_NOMEM = -1, -2, -3, -4
RT_PRECISION_F64, RT_PRECISION_F32 = 0, 1
RT_PIPELINE_AUTO, RT_PIPELINE_MEGAKERNEL, RT_PIPELINE_WAVEFRONT = 0, 1, 2
RT_SCENE_BVH_ON_DEVICE = 1  # RtSceneDesc.flags
RT_MESH_FLAT_SHADING = 1  # RtMesh.flags
RT_MESH_HIT_BACK_FACES = 2
RT_DENOISE_DEMODULATE = 1  # RtDenoiseParams.flags
RT_DENOISE_MAX_ITERATIONS = 16
AOV_CHANNELS = 8  # rt_render_aov: albedo rgb, normal xyz, depth, coverage

(RT_NODE_SPHERE, RT_NODE_PLANE, RT_NODE_MESH, RT_NODE_LIST, RT_NODE_TRANSFORM, RT_NODE_BVH,
 RT_NODE_SKY, RT_NODE_SUN, RT_NODE_VOLUME, RT_NODE_NULL) = range(1, 11)
(RT_MAT_LAMBERTIAN, RT_MAT_METAL, RT_MAT_DIELECTRIC, RT_MAT_GLOSSY, RT_MAT_EMISSIVE,
 RT_MAT_ISOTROPIC, RT_MAT_NORMAL_DEBUG) = range(1, 8)
(RT_TEX_CONST_COLOR, RT_TEX_CONST_FLOAT, RT_TEX_CHECKER, RT_TEX_CHECKER_SOLID, RT_TEX_LERP,
 RT_TEX_IMAGE, RT_TEX_NOISE_SOLID, RT_TEX_CHANNEL, RT_TEX_UV_DEBUG) = range(1, 10)


class RtNode(C.Structure):
    _fields_ = [("type", C.c_uint32), ("flags", C.c_uint32), ("material", C.c_int32),
                ("mesh", C.c_int32), ("transform", C.c_int32), ("first_child", C.c_uint32),
                ("n_children", C.c_uint32), ("_pad", C.c_uint32),
                ("bounds", C.c_double * 6), ("p", C.c_double * 12)]


class RtTransform(C.Structure):
    _fields_ = [("m", C.c_double * 16), ("inv", C.c_double * 16)]


class RtMesh(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_double)), ("normals", C.POINTER(C.c_double)),
                ("uvs", C.POINTER(C.c_double)), ("tri_pos", C.POINTER(C.c_uint32)),
                ("tri_nrm", C.POINTER(C.c_uint32)), ("tri_uv", C.POINTER(C.c_int32)),
                ("n_positions", C.c_uint32), ("n_normals", C.c_uint32), ("n_uvs", C.c_uint32),
                ("n_triangles", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class RtMaterial(C.Structure):
    _fields_ = [("type", C.c_uint32), ("tex_a", C.c_int32), ("tex_b", C.c_int32),
                ("tex_c", C.c_int32), ("ior", C.c_double)]


class RtTexture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32),
                ("channel", C.c_uint32), ("samples", C.c_uint32), ("v", C.c_double * 3),
                ("scale", C.c_double),
                ("texels", C.POINTER(C.c_float)), ("width", C.c_uint32), ("height", C.c_uint32),
                ("perlin_vec", C.POINTER(C.c_double)), ("perlin_perm", C.POINTER(C.c_uint32))]


class RtSceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_nodes", C.c_uint32),
                ("nodes", C.POINTER(RtNode)),
                ("n_child_indices", C.c_uint32), ("n_transforms", C.c_uint32),
                ("child_indices", C.POINTER(C.c_uint32)),
                ("transforms", C.POINTER(RtTransform)),
                ("n_meshes", C.c_uint32), ("n_materials", C.c_uint32),
                ("meshes", C.POINTER(RtMesh)), ("materials", C.POINTER(RtMaterial)),
                ("n_textures", C.c_uint32), ("world_root", C.c_uint32),
                ("textures", C.POINTER(RtTexture)),
                ("lights_root", C.c_uint32), ("flags", C.c_uint32)]


class RtCameraDesc(C.Structure):
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32),
                ("position", C.c_double * 3), ("first_pixel", C.c_double * 3),
                ("pixel_delta_u", C.c_double * 3), ("pixel_delta_v", C.c_double * 3),
                ("basis_u", C.c_double * 3), ("basis_v", C.c_double * 3),
                ("has_aperture", C.c_uint32), ("_pad", C.c_uint32),
                ("aperture_radius", C.c_double)]


class RtRenderParams(C.Structure):
    _fields_ = [("sqrt_spt", C.c_uint32), ("thread_count", C.c_uint32),
                ("max_depth", C.c_uint32), ("has_background", C.c_uint32),
                ("light_bias", C.c_double), ("background", C.c_double * 3),
                ("seed", C.c_uint64),
                ("band_rows", C.c_uint32), ("n_parts", C.c_uint32), ("part", C.c_uint32),
                ("precision", C.c_uint32), ("pipeline", C.c_uint32),
                ("collect_stats", C.c_uint32)]

    def copy(self) -> "RtRenderParams":
        out = RtRenderParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(RtRenderParams))
        return out

    @property
    def spp(self) -> int:
        return self.sqrt_spt * self.sqrt_spt * self.thread_count


class RtRenderStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("traversal_kernel_ms", C.c_double),
                ("n_launches", C.c_uint32), ("pipeline_used", C.c_uint32),
                ("samples", C.c_uint64), ("rays", C.c_uint64), ("mesh_rays", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("prim_tests", C.c_uint64), ("bytes_node", C.c_uint64),
                ("bytes_tri", C.c_uint64), ("bytes_attr", C.c_uint64),
                ("bytes_state", C.c_uint64),
                ("prims_kernel_ms", C.c_double), ("shade_kernel_ms", C.c_double),
                ("bytes_state_prims", C.c_uint64), ("bytes_state_shade", C.c_uint64),
                ("n_iterations", C.c_uint32), ("n_replica_groups", C.c_uint32),
                ("n_tail_compactions", C.c_uint32), ("_reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class RtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("aov_replicas", C.c_uint32), ("flags", C.c_uint32),
                ("_reserved0", C.c_uint32), ("sigma_color", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_albedo", C.c_double), ("sigma_depth", C.c_double), ("_reserved", C.c_double * 4)]

    @classmethod
    def defaults(cls, **overrides) -> "RtDenoiseParams":
        """rt_denoise_default_params, then the given fields."""
        dp = cls()
        load_device_lib().rt_denoise_default_params(C.byref(dp))
        for name, value in overrides.items():
            setattr(dp, name, value)
        return dp


class RtAdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("floor", C.c_double), ("min_replicas", C.c_uint32),
                ("check_interval", C.c_uint32), ("radius", C.c_uint32), ("_reserved0", C.c_uint32),
                ("_reserved", C.c_double * 4)]

    @classmethod
    def defaults(cls, **overrides) -> "RtAdaptiveParams":
        """rt_adaptive_default_params, then the given fields (`threshold` has no default and must be given)."""
        ap = cls()
        load_device_lib().rt_adaptive_default_params(C.byref(ap))
        for name, value in overrides.items():
            setattr(ap, name, value)
        return ap


RT_LIGHT_GROUPS_MAX = 16


class RtLightGroups(C.Structure):
    """include/rt_mi355.h RtLightGroups; `make` keeps the byte table alive with the structure."""
    _fields_ = [("n_groups", C.c_uint32), ("n_materials", C.c_uint32), ("material_group", C.POINTER(C.c_uint8)),
                ("background_group", C.c_uint32), ("unlit_group", C.c_uint32), ("_reserved", C.c_uint32 * 4)]

    @classmethod
    def make(cls, n_groups: int, material_group, background_group: int = 0, unlit_group: int = 0) -> "RtLightGroups":
        table = np.ascontiguousarray(material_group, dtype=np.uint8).copy()
        g = cls()
        g.n_groups, g.n_materials = n_groups, table.size
        g.material_group = table.ctypes.data_as(C.POINTER(C.c_uint8))
        g.background_group, g.unlit_group = background_group, unlit_group
        g._table = table
        return g

    @property
    def table(self) -> np.ndarray:
        return self._table


class RtSceneUpdateInfo(C.Structure):
    """include/rt_mi355.h RtSceneUpdateInfo: what an rt_scene_update did."""
    _fields_ = [("n_meshes_refit", C.c_uint32), ("n_triangles_refit", C.c_uint32), ("bytes_uploaded", C.c_uint64),
                ("refit_kernel_ms", C.c_double), ("total_ms", C.c_double), ("_reserved", C.c_uint32 * 4)]


class RtRayQueryStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("rays", C.c_uint64), ("n_chunks", C.c_uint32), ("precision", C.c_uint32),
                ("_reserved", C.c_uint32 * 4)]


# RtRayHit (include/rt_mi355.h) as a numpy structured dtype: DeviceScene.trace_rays returns an array of it
RT_RAY_HIT, RT_RAY_FRONT_FACE, RT_RAY_ENVIRONMENT = 1, 2, 4
RtRayHit = np.dtype([("t", "<f8"), ("pos", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("material", "<i4"),
                     ("node", "<i4"), ("prim", "<i4"), ("flags", "<u4"), ("_reserved", "<u8")])
assert RtRayHit.itemsize == 96

# RtPointHit (include/rt_mi355.h) as a numpy structured dtype: DeviceScene.closest_points returns an array of it
RT_POINT_FOUND, RT_POINT_BACK_SIDE = 1, 2
RtPointHit = np.dtype([("distance", "<f8"), ("pos", "<f8", (3,)), ("normal", "<f8", (3,)), ("material", "<i4"), ("node", "<i4"),
                       ("prim", "<i4"), ("flags", "<u4"), ("_reserved", "<u8")])
assert RtPointHit.itemsize == 80


class RtBakeParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("precision", C.c_uint32), ("seed", C.c_uint64), ("bias", C.c_double),
                ("max_distance", C.c_double), ("_reserved", C.c_uint32 * 4)]

    @classmethod
    def defaults(cls, **overrides) -> "RtBakeParams":
        p = cls(samples=64, precision=RT_PRECISION_F64, seed=0, bias=1e-3, max_distance=float("inf"))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


# RtBakeResult (include/rt_mi355.h) as a numpy structured dtype: DeviceScene.bake_visibility returns an array of it
RtBakeResult = np.dtype([("visibility", "<f8"), ("bent", "<f8", (3,))])
assert RtBakeResult.itemsize == 32


class RtLightmapStats(C.Structure):
    """include/rt_mi355.h RtLightmapStats: the last rasterisation of a lightmap on a scene."""
    _fields_ = [("bin_ms", C.c_double), ("raster_ms", C.c_double), ("texels", C.c_uint64), ("covered_texels", C.c_uint64),
                ("tile_refs", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("_reserved", C.c_uint32 * 4)]


RT_LIGHTMAP_IRRADIANCE, RT_LIGHTMAP_VISIBILITY = 0, 1
_LIGHTMAP_KINDS = {"irradiance": RT_LIGHTMAP_IRRADIANCE, "visibility": RT_LIGHTMAP_VISIBILITY}


class RtError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"rt status {status}: {message}")
        self.status = status


HOST_LIB_PATH = os.path.join(PKG_DIR, "librt_host.so")
DEVICE_LIB_PATH = os.environ.get("RT_DEVICE_LIB") or os.path.join(PKG_DIR, "librt_mi355.so")  # env override: A/B builds

_host_lib = None
_device_lib = None


def _check(lib, st: int) -> None:
    """Raises RtError with the last error text of `lib` (the device library, or the host library) unless st is RT_OK."""
    if st != RT_OK:
        raise RtError(st, (lib.rth_last_error if lib is _host_lib else lib.rt_last_error)().decode())


def _table(a, name: str) -> np.ndarray:
    """`a` as an (n, 3) float64 C-contiguous table; a single (3,) entry becomes (1, 3).  `name`: of the argument(s), in errors."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1:] != (3,) or a.ndim > 2:
        raise ValueError(f"{name} must be (n, 3) or (3,)")
    return np.ascontiguousarray(np.atleast_2d(a))


def load_host_lib() -> C.CDLL:
    global _host_lib
    if _host_lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise FileNotFoundError(
                f"{HOST_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(HOST_LIB_PATH)
        lib.rth_load.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
        lib.rth_load.restype = C.c_int
        lib.rth_destroy.argtypes = [C.c_void_p]
        lib.rth_destroy.restype = None
        lib.rth_scene.argtypes = [C.c_void_p]
        lib.rth_scene.restype = C.POINTER(RtSceneDesc)
        lib.rth_camera.argtypes = [C.c_void_p]
        lib.rth_camera.restype = C.POINTER(RtCameraDesc)
        lib.rth_params.argtypes = [C.c_void_p]
        lib.rth_params.restype = C.POINTER(RtRenderParams)
        lib.rth_gpus.argtypes = [C.c_void_p]
        lib.rth_gpus.restype = C.c_uint32
        lib.rth_band_rows.argtypes = [C.c_uint32, C.c_uint32]
        lib.rth_band_rows.restype = C.c_uint32
        lib.rth_samples_per_pixel.argtypes = [C.c_void_p]
        lib.rth_samples_per_pixel.restype = C.c_uint32
        lib.rth_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.rth_pick.restype = C.c_uint32
        lib.rth_ao.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.rth_ao.restype = C.c_uint32
        lib.rth_irradiance.argtypes = [C.c_void_p]
        lib.rth_irradiance.restype = C.c_int
        lib.rth_sh_probes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.rth_sh_probes.restype = C.c_uint32
        lib.rth_nearest_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.rth_nearest_points.restype = C.c_uint32
        lib.rth_probe.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.rth_probe.restype = C.c_uint32
        lib.rth_probe_rays.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.rth_probe_rays.restype = C.c_int
        lib.rth_log.argtypes = [C.c_void_p]
        lib.rth_log.restype = C.c_char_p
        lib.rth_make_camera.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(RtCameraDesc)]
        lib.rth_make_camera.restype = C.c_int
        lib.rth_tonemap_rgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rth_tonemap_rgb8.restype = C.c_int
        lib.rth_save_png.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.rth_save_png.restype = C.c_int
        lib.rth_load_image.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.rth_load_image.restype = C.c_int
        lib.rth_free_image.argtypes = [C.POINTER(C.c_float)]
        lib.rth_free_image.restype = None
        lib.rth_last_error.argtypes = []
        lib.rth_last_error.restype = C.c_char_p
        _host_lib = lib
    return _host_lib


def load_device_lib() -> C.CDLL:
    """Loads the HIP library.  Raises if it has not been built: there is no fallback."""
    global _device_lib
    if _device_lib is None:
        if not os.path.exists(DEVICE_LIB_PATH):
            raise FileNotFoundError(
                f"{DEVICE_LIB_PATH} is missing — the HIP render path was not built "
                "(run __graft_entry__.build()); refusing to fall back to any CPU path")
        # A process that also uses PyTorch must load PyTorch's HIP runtime FIRST: the wheel bundles its own
        # libamdhip64, and if the system copy (our dependency) is already loaded, torch then sees "No HIP GPUs".
        # Loaded in this order, both share torch's copy.  (Pure C / C++ callers are not affected.)
        if "torch" not in sys.modules and os.environ.get("RT_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # PyTorch absent or broken: the library works on its own
                pass
        lib = C.CDLL(DEVICE_LIB_PATH)
        lib.rt_device_count.argtypes = []
        lib.rt_device_count.restype = C.c_int
        lib.rt_scene_create.argtypes = [C.POINTER(RtSceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        lib.rt_scene_create.restype = C.c_int
        lib.rt_scene_destroy.argtypes = [C.c_void_p]
        lib.rt_scene_destroy.restype = None
        lib.rt_owned_rows.argtypes = [C.c_uint32, C.POINTER(RtRenderParams)]
        lib.rt_owned_rows.restype = C.c_uint32
        lib.rt_render.argtypes = [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), C.c_void_p]
        lib.rt_render.restype = C.c_int
        lib.rt_render_device.argtypes = [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                         C.c_void_p, C.c_void_p]
        lib.rt_render_device.restype = C.c_int
        lib.rt_get_stats.argtypes = [C.c_void_p, C.POINTER(RtRenderStats)]
        lib.rt_get_stats.restype = C.c_int
        lib.rt_debug_trace_sample.argtypes = [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                              C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32]
        lib.rt_debug_trace_sample.restype = C.c_int
        if hasattr(lib, "rt_debug_shade_rays"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_debug_shade_rays.argtypes = [C.c_void_p, C.POINTER(RtRenderParams), C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
            lib.rt_debug_shade_rays.restype = C.c_int
        lib.rt_scene_info.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(C.c_uint32)]
        lib.rt_scene_info.restype = C.c_int
        if hasattr(lib, "rt_scene_set_tail_flag"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_scene_set_tail_flag.argtypes = [C.c_void_p, C.c_void_p]
            lib.rt_scene_set_tail_flag.restype = C.c_int
        if hasattr(lib, "rt_scene_mesh_stats"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_scene_mesh_stats.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(C.c_uint64)]
            lib.rt_scene_mesh_stats.restype = C.c_int
        if hasattr(lib, "rt_scene_tables_digest"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_scene_tables_digest.argtypes = [C.POINTER(RtSceneDesc), C.c_uint32, C.POINTER(C.c_uint64)]
            lib.rt_scene_tables_digest.restype = C.c_int
        if hasattr(lib, "rt_scene_mesh_cones"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_scene_mesh_cones.argtypes = [C.POINTER(RtSceneDesc), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
            lib.rt_scene_mesh_cones.restype = C.c_int
        if hasattr(lib, "rt_scene_mesh_slabs"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_scene_mesh_slabs.argtypes = [C.POINTER(RtSceneDesc), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]
            lib.rt_scene_mesh_slabs.restype = C.c_int
        if hasattr(lib, "rt_debug_handout_replay"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_debug_handout_replay.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.POINTER(C.c_uint32), C.c_void_p]
            lib.rt_debug_handout_replay.restype = C.c_int
        if hasattr(lib, "rt_accum_create"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            for name, res, args in (
                    ("rt_accum_create", C.c_int, [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), C.POINTER(C.c_void_p)]),
                    ("rt_accum_destroy", None, [C.c_void_p]),
                    ("rt_accum_render", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RtRenderParams), C.c_void_p]),
                    ("rt_accum_replicas_done", C.c_uint32, [C.c_void_p]),
                    ("rt_accum_estimate", C.c_int, [C.c_void_p, C.c_void_p]),
                    ("rt_accum_estimate_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
                    ("rt_accum_preview_rgb8", C.c_int, [C.c_void_p, C.c_void_p]),
                    ("rt_accum_state_size", C.c_size_t, [C.c_void_p]),
                    ("rt_accum_save_state", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
                    ("rt_accum_load_state", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
                    ("rt_tonemap_rgb8_device", C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_render_aov"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            dp = C.POINTER(RtDenoiseParams)
            for name, res, args in (
                    ("rt_render_aov", C.c_int, [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), C.c_uint32, C.c_void_p]),
                    ("rt_render_aov_device", C.c_int, [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), C.c_uint32,
                                                       C.c_void_p, C.c_void_p]),
                    ("rt_denoise_default_params", C.c_int, [dp]),
                    ("rt_denoise", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, dp, C.c_void_p]),
                    ("rt_denoise_device", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, dp, C.c_void_p, C.c_void_p]),
                    ("rt_accum_estimate_denoised", C.c_int, [C.c_void_p, dp, C.c_void_p]),
                    ("rt_accum_preview_denoised_rgb8", C.c_int, [C.c_void_p, dp, C.c_void_p])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_accum_set_adaptive"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            for name, res, args in (
                    ("rt_adaptive_default_params", C.c_int, [C.POINTER(RtAdaptiveParams)]),
                    ("rt_accum_set_adaptive", C.c_int, [C.c_void_p, C.POINTER(RtAdaptiveParams)]),
                    ("rt_accum_active_pixels", C.c_uint32, [C.c_void_p]),
                    ("rt_accum_finished", C.c_int, [C.c_void_p]),
                    ("rt_accum_sample_counts", C.c_int, [C.c_void_p, C.c_void_p]),
                    ("rt_accum_noise", C.c_int, [C.c_void_p, C.c_void_p])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_render_light_groups"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lg = C.POINTER(RtLightGroups)
            for name, res, args in (
                    ("rt_light_groups_auto", C.c_int, [C.POINTER(RtSceneDesc), C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint32),
                                                       C.POINTER(C.c_uint32)]),
                    ("rt_render_light_groups", C.c_int, [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), lg, C.c_void_p,
                                                         C.c_void_p]),
                    ("rt_render_light_groups_device", C.c_int, [C.c_void_p, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), lg,
                                                                C.c_void_p, C.c_void_p, C.c_void_p]),
                    ("rt_light_mix", C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
                    ("rt_light_mix_device", C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                      C.c_void_p])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_scene_update"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            mesh_out = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_uint32,
                        C.POINTER(C.c_uint32)]
            for name, res, args in (
                    ("rt_scene_update", C.c_int, [C.c_void_p, C.POINTER(RtSceneDesc), C.POINTER(RtSceneUpdateInfo)]),
                    ("rt_scene_update_check", C.c_int, [C.POINTER(RtSceneDesc), C.POINTER(RtSceneDesc)]),
                    ("rt_scene_refit_mesh", C.c_int, [C.POINTER(RtSceneDesc), C.POINTER(RtSceneDesc), C.c_uint32, C.c_uint32] + mesh_out),
                    ("rt_debug_scene_mesh", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32] + mesh_out),
                    ("rt_debug_scene_mesh_digest", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_trace_rays"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            for name, res, args in (
                    ("rt_trace_rays", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
                    ("rt_trace_rays_device", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
                    ("rt_occluded", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
                    ("rt_occluded_device", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_void_p]),
                    ("rt_ray_query_stats", C.c_int, [C.c_void_p, C.POINTER(RtRayQueryStats)]),
                    ("rt_scene_op_nodes", C.c_int, [C.POINTER(RtSceneDesc), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_closest_points"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            for name, res, args in (
                    ("rt_closest_points", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
                    ("rt_closest_points_device", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
                    ("rt_point_query_stats", C.c_int, [C.c_void_p, C.POINTER(RtRayQueryStats)]),
                    ("rt_debug_closest_points_counts", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_bake_visibility"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            for name, res, args in (
                    ("rt_bake_visibility", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtBakeParams), C.c_void_p]),
                    ("rt_bake_visibility_device", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtBakeParams),
                                                            C.c_void_p, C.c_void_p]),
                    ("rt_bake_visibility_hits_device", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtBakeParams), C.c_void_p,
                                                                 C.c_void_p]),
                    ("rt_bake_stats", C.c_int, [C.c_void_p, C.POINTER(RtRayQueryStats)])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_render_rays"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_render_rays.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p]
            lib.rt_render_rays.restype = C.c_int
            lib.rt_render_rays_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p,
                                                  C.c_void_p]
            lib.rt_render_rays_device.restype = C.c_int
        if hasattr(lib, "rt_bake_irradiance"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_bake_irradiance.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p]
            lib.rt_bake_irradiance.restype = C.c_int
            lib.rt_bake_irradiance_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p,
                                                      C.c_void_p]
            lib.rt_bake_irradiance_device.restype = C.c_int
            lib.rt_bake_irradiance_hits_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p, C.c_void_p]
            lib.rt_bake_irradiance_hits_device.restype = C.c_int
        if hasattr(lib, "rt_bake_probes"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_bake_probes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p]
            lib.rt_bake_probes.restype = C.c_int
            lib.rt_bake_probes_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtRenderParams), C.c_void_p, C.c_void_p]
            lib.rt_bake_probes_device.restype = C.c_int
            lib.rt_sh_irradiance.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            lib.rt_sh_irradiance.restype = C.c_int
            lib.rt_sh_irradiance_device.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
            lib.rt_sh_irradiance_device.restype = C.c_int
        if hasattr(lib, "rt_lightmap_texels"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            u32, vp = C.c_uint32, C.c_void_p
            for name, res, args in (
                    ("rt_lightmap_texels", C.c_int, [vp, u32, u32, u32, u32, vp, vp]),
                    ("rt_lightmap_texels_device", C.c_int, [vp, u32, u32, u32, u32, vp, vp, vp]),
                    ("rt_lightmap_texels_desc", C.c_int, [C.POINTER(RtSceneDesc), u32, u32, u32, u32, vp, vp]),
                    ("rt_lightmap_dilate", C.c_int, [C.c_int, vp, vp, u32, u32, C.c_int32, vp, vp]),
                    ("rt_lightmap_dilate_device", C.c_int, [C.c_int, vp, vp, u32, u32, C.c_int32, vp, vp, vp]),
                    ("rt_bake_lightmap", C.c_int, [vp, u32, u32, u32, u32, u32, C.POINTER(RtRenderParams), C.POINTER(RtBakeParams), C.c_int32, vp, vp]),
                    ("rt_bake_lightmap_device", C.c_int, [vp, u32, u32, u32, u32, u32, C.POINTER(RtRenderParams), C.POINTER(RtBakeParams), C.c_int32,
                                                          vp, vp, vp]),
                    ("rt_lightmap_stats", C.c_int, [vp, C.POINTER(RtLightmapStats)])):
                fn = getattr(lib, name)
                fn.argtypes = args
                fn.restype = res
        if hasattr(lib, "rt_debug_live_resources"):  # absent from older A/B builds loaded through RT_DEVICE_LIB
            lib.rt_debug_live_resources.argtypes = [C.POINTER(C.c_uint64)]
            lib.rt_debug_live_resources.restype = C.c_int
        lib.rt_last_error.argtypes = []
        lib.rt_last_error.restype = C.c_char_p
        _device_lib = lib
    return _device_lib


RT_SCENE_INFO_ZERO_WEIGHT_STOP, RT_SCENE_INFO_TEX_INTERPRETER, RT_SCENE_INFO_VOLUMES = 1, 2, 4


def scene_info(desc) -> int:
    """rt_scene_info: the scene compiler's classification flags (host only, no device needed)."""
    lib = load_device_lib()
    flags = C.c_uint32()
    st = lib.rt_scene_info(desc, C.byref(flags))
    _check(lib, st)
    return flags.value


def scene_mesh_stats(desc) -> dict:
    """rt_scene_mesh_stats: triangle records / BVH node counts / depths (host only)."""
    lib = load_device_lib()
    out = (C.c_uint64 * 8)()
    st = lib.rt_scene_mesh_stats(desc, out)
    _check(lib, st)
    return dict(zip(("triangles", "bvh2_nodes", "bvh4_nodes", "bvh2_depth", "bvh4_stack", "ops", "rebuilt_groups", "rebuilt_prims"),
                    [int(x) for x in out]))


def scene_tables_digest(desc, f32: bool = False) -> tuple:
    """rt_scene_tables_digest: digests of the seven mesh tables as the host derives them for DeviceScene(desc), in the order
    of DeviceScene.debug_mesh_digest (whose first seven entries they equal once the tables are on the device); the eighth is
    0.  Host only."""
    lib = load_device_lib()
    out = (C.c_uint64 * 8)()
    st = lib.rt_scene_tables_digest(desc, int(f32), out)
    _check(lib, st)
    return tuple(int(x) for x in out)


def lightmap_texels_desc(desc, node: int, width: int, height: int, instance: int = 0, counts: bool = False):
    """rt_lightmap_texels_desc: the texel rule of DeviceScene.lightmap_texels by brute force on the host, from the description
    alone (no device needed): (height, width) api.RtRayHit records, and with counts=True also the (height, width) uint32 number
    of covering triangles per texel."""
    lib = load_device_lib()
    hits = np.zeros((max(height, 0), max(width, 0)) if 0 < width <= 16384 and 0 < height <= 16384 else (1, 1), dtype=RtRayHit)
    cnt = np.zeros(hits.shape, dtype=np.uint32) if counts else None
    st = lib.rt_lightmap_texels_desc(desc, node, instance, width, height, hits.ctypes.data, None if cnt is None else cnt.ctypes.data)
    _check(lib, st)
    return (hits, cnt) if counts else hits


def lightmap_dilate(rgba, coverage, passes: int = 2, device: int = 0) -> tuple:
    """rt_lightmap_dilate: `passes` dilation passes of an (h, w, 4) float64 image with its (h, w) coverage (non-zero = covered):
    an uncovered texel next to covered ones takes their mean and counts as covered from then on.  Returns (rgba, coverage)."""
    lib = load_device_lib()
    img = np.ascontiguousarray(rgba, dtype=np.float64)
    cov = np.ascontiguousarray(coverage, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 4 or cov.shape != img.shape[:2]:
        raise ValueError("lightmap_dilate: rgba must be (h, w, 4) and coverage (h, w)")
    out, out_c = np.zeros_like(img), np.zeros_like(cov)
    st = lib.rt_lightmap_dilate(device, img.ctypes.data, cov.ctypes.data, img.shape[1], img.shape[0], passes, out.ctypes.data, out_c.ctypes.data)
    _check(lib, st)
    return out, out_c


def live_resources() -> tuple:
    """rt_debug_live_resources: (live device buffers, their bytes, live pinned host buffers, live events + streams) that the
    library holds in this process."""
    lib = load_device_lib()
    out = (C.c_uint64 * 4)()
    st = lib.rt_debug_live_resources(out)
    _check(lib, st)
    return tuple(int(x) for x in out)


def handout_replay(n: int, waves: int, order, policy=None, out=None) -> tuple:
    """rt_debug_handout_replay: the ranges the persistent search kernels' hand-out policy gives `waves` waves that ask in `order`
    (walked round and round) for a queue of n entries -> (asks (k, 3) uint32: wave, first, end; 0xFFFFFFFF twice = "exhausted",
    atomics of the kernel, atomics of the asks after "exhausted").  `out`: a (cap, 3) uint32 array to reuse."""
    lib = load_device_lib()
    order = np.ascontiguousarray(order, dtype=np.uint32)
    pol = None if policy is None else np.asarray(policy, dtype=np.uint32)
    cap = n // 64 + 4 * waves + 16
    if out is None or out.shape[0] < cap:
        out = np.empty((cap, 3), dtype=np.uint32)
    n_asks = C.c_uint32(0)
    atomics = np.zeros(2, dtype=np.uint32)
    st = lib.rt_debug_handout_replay(None if pol is None else pol.ctypes.data, n, waves, order.ctypes.data, order.size, out.ctypes.data,
                                     out.shape[0], C.byref(n_asks), atomics.ctypes.data)
    if st != 0:
        raise RuntimeError(f"rt_debug_handout_replay: {lib.rt_last_error().decode()}")
    if n_asks.value > out.shape[0]:
        raise RuntimeError(f"rt_debug_handout_replay: {n_asks.value} asks for n = {n}, {waves} waves")
    return out[:n_asks.value], int(atomics[0]), int(atomics[1])


def scene_mesh_cones(desc, mesh: int = 0, f32: bool = False) -> tuple:
    """rt_scene_mesh_cones: (children (n, 4) int32, cone words (n, 4, 4) int8 as (ax, ay, az, w), triangle records (t, 3, 3)
    float64 as (v0, e1, e2) in leaf order) of mesh instance `mesh`; host only."""
    import numpy as np
    lib = load_device_lib()
    nn, nt = C.c_uint32(), C.c_uint32()
    st = lib.rt_scene_mesh_cones(desc, mesh, int(f32), None, None, 0, C.byref(nn), None, 0, C.byref(nt))
    _check(lib, st)
    children = np.zeros((nn.value, 4), dtype=np.int32)
    cones = np.zeros((nn.value, 4), dtype=np.uint32)
    tris = np.zeros((nt.value, 3, 3), dtype=np.float64)
    st = lib.rt_scene_mesh_cones(desc, mesh, int(f32), children.ctypes.data, cones.ctypes.data, nn.value, C.byref(nn),
                                 tris.ctypes.data, nt.value, C.byref(nt))
    _check(lib, st)
    return children, cones.view(np.int8).reshape(-1, 4, 4), tris


def scene_mesh_slabs(desc, mesh: int = 0, f32: bool = False) -> dict:
    """rt_scene_mesh_slabs, for the nodes of scene_mesh_cones in the same order: {"words" (n, 4) uint32, "bounds" (n, 4, 2)
    float32 as (lo, hi), "org" (n, 3) float32, "inv_s" (n,) float32, "pad" float}; host only."""
    import numpy as np
    lib = load_device_lib()
    nn, pad = C.c_uint32(), C.c_double()
    st = lib.rt_scene_mesh_slabs(desc, mesh, int(f32), None, None, None, C.byref(pad), 0, C.byref(nn))
    _check(lib, st)
    words = np.zeros((nn.value, 4), dtype=np.uint32)
    bounds = np.zeros((nn.value, 4, 2), dtype=np.float32)
    frames = np.zeros((nn.value, 4), dtype=np.float32)
    st = lib.rt_scene_mesh_slabs(desc, mesh, int(f32), words.ctypes.data, bounds.ctypes.data, frames.ctypes.data, C.byref(pad),
                                 nn.value, C.byref(nn))
    _check(lib, st)
    return {"words": words, "bounds": bounds, "org": frames[:, :3].copy(), "inv_s": frames[:, 3].copy(), "pad": float(pad.value)}


def scene_update_check(a, b) -> None:
    """rt_scene_update_check: raises RtError (RT_E_INVALID, naming the first field that differs) unless description `b` has
    the structure of `a`, i.e. unless DeviceScene(a).update(b) would be accepted as far as the structure goes; host only."""
    lib = load_device_lib()
    st = lib.rt_scene_update_check(a, b)
    _check(lib, st)


def _mesh_export(call) -> dict:
    """The outputs shared by rt_scene_refit_mesh and rt_debug_scene_mesh; call(children, cones, boxes, node capacity, n_nodes,
    tris, order, triangle capacity, n_tris) -> status."""
    lib = load_device_lib()
    nn, nt = C.c_uint32(), C.c_uint32()
    st = call(None, None, None, 0, C.byref(nn), None, None, 0, C.byref(nt))
    _check(lib, st)
    children = np.zeros((nn.value, 4), dtype=np.int32)
    cones = np.zeros((nn.value, 4), dtype=np.uint32)
    boxes = np.zeros((nn.value, 4, 2, 3), dtype=np.float32)
    tris = np.zeros((nt.value, 3, 3), dtype=np.float64)
    order = np.zeros(nt.value, dtype=np.uint32)
    st = call(children.ctypes.data, cones.ctypes.data, boxes.ctypes.data, nn.value, C.byref(nn), tris.ctypes.data, order.ctypes.data,
              nt.value, C.byref(nt))
    _check(lib, st)
    return {"children": children, "cones": cones.view(np.int8).reshape(-1, 4, 4), "boxes": boxes, "tris": tris, "order": order}


def scene_refit_mesh(a, b, mesh: int = 0, f32: bool = False) -> dict:
    """rt_scene_refit_mesh: the refit on the CPU (host only, through the derivation that fills the device): the tree DeviceScene(a) builds for mesh instance
    `mesh`, carrying the geometry of `b`.  {"children" (n, 4) int32, "cones" (n, 4, 4) int8, "boxes" (n, 4, 2, 3) float32
    decoded quantised child boxes (lo, hi; empty child: lo > hi), "tris" (t, 3, 3) float64 (v0, e1, e2 in the kernels'
    arithmetic type), "order" (t,) uint32 leaf slot -> original triangle}."""
    lib = load_device_lib()
    return _mesh_export(lambda *out: lib.rt_scene_refit_mesh(a, b, mesh, int(f32), *out))


def scene_program(desc) -> tuple:
    """rt_scene_program: (ops as an (n, 4) int32 array of type / arg / skip / chain, info dict); host only."""
    import numpy as np
    lib = load_device_lib()
    lib.rt_scene_program.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.rt_scene_program.restype = C.c_int
    n = C.c_uint32()
    info = (C.c_uint64 * 8)()
    st = lib.rt_scene_program(desc, None, 0, C.byref(n), info)
    _check(lib, st)
    ops = np.zeros((n.value, 4), dtype=np.int32)
    st = lib.rt_scene_program(desc, ops.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n), info)
    _check(lib, st)
    plan = int(info[6])
    return ops, {"mesh_ops": int(info[0]), "groups": int(info[1]), "group_nodes": int(info[2]), "group_stack": int(info[3]),
                 "lights": int(info[4]), "volumes": int(info[5]), "group_prims": int(info[7]),
                 "split": bool(plan & 1), "vol_prims": bool(plan & 2), "multi_mesh": bool(plan & 4), "group_bvh": bool(plan & 8)}


def scene_groups(desc, f32: bool = False) -> dict:
    """rt_scene_groups: the 4-wide BVHs of the re-built primitive groups as k_wf_prims reads them (host only, through the
    derivation that fills the device).  {"roots" (g,) uint32 and "group_boxes" (g, 2, 3) float64 (lo, hi) per group; "children"
    (n, 4) int32 absolute child references and "boxes" (n, 4, 2, 3) float32 decoded quantised child boxes (lo, hi; no child:
    lo > hi) per node; "prims" (p, 3) int32 as (pc, guard_first, guard_count) per position of the primitive array; "guards" (q,)
    int32, the guard array; "stack_levels": levels per lane that k_wf_prims is given; "n_bounds": entries of the bounds table}."""
    lib = load_device_lib()
    lib.rt_scene_groups.argtypes = [C.POINTER(RtSceneDesc), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.rt_scene_groups.restype = C.c_int
    counts = (C.c_uint32 * 6)()
    st = lib.rt_scene_groups(desc, int(f32), None, None, 0, None, None, 0, None, 0, None, 0, counts)
    _check(lib, st)
    ng, nn, npr, nq = (int(counts[k]) for k in range(4))
    roots, gboxes = np.zeros(ng, dtype=np.uint32), np.zeros((ng, 2, 3), dtype=np.float64)
    children, boxes = np.zeros((nn, 4), dtype=np.int32), np.zeros((nn, 4, 2, 3), dtype=np.float32)
    prims, guards = np.zeros((npr, 3), dtype=np.int32), np.zeros(nq, dtype=np.int32)
    st = lib.rt_scene_groups(desc, int(f32), roots.ctypes.data, gboxes.ctypes.data, ng, children.ctypes.data, boxes.ctypes.data, nn,
                             prims.ctypes.data, npr, guards.ctypes.data, nq, counts)
    _check(lib, st)
    return {"roots": roots, "group_boxes": gboxes, "children": children, "boxes": boxes, "prims": prims, "guards": guards,
            "stack_levels": int(counts[4]), "n_bounds": int(counts[5])}


def scene_op_nodes(desc) -> np.ndarray:
    """rt_scene_op_nodes: per op of the compiled program (api.scene_program order) the RtSceneDesc.nodes index it came from,
    -1 for ops that belong to no single node; host only."""
    lib = load_device_lib()
    n = C.c_uint32()
    st = lib.rt_scene_op_nodes(desc, None, 0, C.byref(n))
    _check(lib, st)
    nodes = np.full(n.value, -1, dtype=np.int32)
    st = lib.rt_scene_op_nodes(desc, nodes.ctypes.data, n.value, C.byref(n))
    _check(lib, st)
    return nodes


def light_groups_auto(desc, max_groups: int = RT_LIGHT_GROUPS_MAX, has_background: bool = False) -> RtLightGroups:
    """rt_light_groups_auto (host only): group 0 = unlit and everything that does not emit, one group per Emissive material
    of `world` in material order, then the background; ids beyond max_groups - 1 share that id."""
    lib = load_device_lib()
    d = desc.contents if hasattr(desc, "contents") else desc
    table = np.zeros(d.n_materials, dtype=np.uint8)
    bg, n = C.c_uint32(), C.c_uint32()
    st = lib.rt_light_groups_auto(desc, max_groups, int(bool(has_background)), table.ctypes.data, C.byref(bg), C.byref(n))
    _check(lib, st)
    return RtLightGroups.make(n.value, table, bg.value, 0)


def light_mix(groups: np.ndarray, tints, device: int = 0) -> np.ndarray:
    """rt_light_mix: (G, H, W, 4) group frames and G x 3 tints (or G scalars) -> the (H, W, 4) re-mixed frame, on the GPU."""
    lib = load_device_lib()
    groups = np.ascontiguousarray(groups, dtype=np.float64)
    if groups.ndim != 4 or groups.shape[3] != 4:
        raise ValueError(f"light_mix: expected a (G, H, W, 4) array, got {groups.shape}")
    g, h, w = groups.shape[:3]
    tints = np.asarray(tints, dtype=np.float64)
    if tints.ndim == 1:
        tints = np.repeat(tints[:, None], 3, axis=1)
    tints = np.ascontiguousarray(tints)
    if tints.shape != (g, 3):
        raise ValueError(f"light_mix: expected {g} x 3 tints, got {tints.shape}")
    out = np.empty((h, w, 4), dtype=np.float64)
    st = lib.rt_light_mix(device, groups.ctypes.data, g, w, h, tints.ctypes.data, out.ctypes.data)
    _check(lib, st)
    return out


def probe_grid(lo, hi, counts) -> np.ndarray:
    """Cell-centred positions of an irradiance volume: the box lo .. hi cut into counts = (nx, ny, nz) cells, x fastest; position
    (ix, iy, iz) = lo + (hi - lo) * ((i + 0.5) / counts) per axis, at index (iz * ny + iy) * nx + ix.  (nx * ny * nz, 3) float64."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    counts = np.asarray(counts)
    if lo.shape != (3,) or hi.shape != (3,) or counts.shape != (3,) or counts.dtype.kind not in "iu" or (counts < 1).any():
        raise ValueError("probe_grid: lo and hi must be (3,), counts three positive integers")
    axes = [lo[a] + (hi[a] - lo[a]) * ((np.arange(int(counts[a]), dtype=np.float64) + 0.5) / float(counts[a])) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))


def sh_irradiance(sh, probe, normals, device: int = 0) -> np.ndarray:
    """rt_sh_irradiance: lighting from SH probes.  sh: (n, 9, 4) from DeviceScene.bake_probes; probe: (m,) indices below n (or one
    index); normals: (m, 3) or (3,), need not be unit length.  Returns (m, 4) float64, (r, g, b, 0): the clamped-cosine
    convolution of the probe's radiance divided by pi - the unit of bake_irradiance, irradiance = pi * out."""
    lib = load_device_lib()
    sh = np.ascontiguousarray(sh, dtype=np.float64)
    if sh.ndim != 3 or sh.shape[1:] != (9, 4):
        raise ValueError(f"sh_irradiance: expected an (n, 9, 4) array, got {sh.shape}")
    idx = np.asarray(probe)
    if idx.dtype.kind not in "iu" or ((idx < 0) | (idx > 0xFFFFFFFF)).any():
        raise ValueError("sh_irradiance: probe indices must be integers in 0 .. 2^32 - 1")
    nr = np.asarray(normals, dtype=np.float64)
    if nr.shape[-1:] != (3,) or nr.ndim > 2 or idx.ndim > 1:
        raise ValueError("sh_irradiance: probe must be (m,) or a single index, normals (m, 3) or (3,)")
    m = max(idx.size if idx.ndim else 1, len(nr) if nr.ndim == 2 else 1)
    idx = np.ascontiguousarray(np.broadcast_to(idx.astype(np.uint32), (m,)))
    nr = np.ascontiguousarray(np.broadcast_to(nr, (m, 3)))
    out = np.empty((m, 4), dtype=np.float64)
    st = lib.rt_sh_irradiance(device, sh.ctypes.data, len(sh), idx.ctypes.data, nr.ctypes.data, m, out.ctypes.data)
    _check(lib, st)
    return out


def sh_irradiance_device(d_sh_ptr: int, n_probes: int, d_probe_ptr: int, d_normals_ptr: int, m: int, d_out_ptr: int, device: int = 0,
                         stream: int = 0) -> None:
    """rt_sh_irradiance_device: n_probes x 9 x 4 doubles, m uint32 indices and m x 3 doubles in HBM -> m x 4 doubles in HBM; an index
    out of range gives (0, 0, 0, 0)."""
    lib = load_device_lib()
    st = lib.rt_sh_irradiance_device(device, C.c_void_p(d_sh_ptr or None), n_probes, C.c_void_p(d_probe_ptr or None), C.c_void_p(d_normals_ptr or None),
                                     m, C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
    _check(lib, st)


def owned_rows(height: int, params: RtRenderParams) -> list:
    """Rows of the frame that the partition in `params` assigns to this part (rt_owned_rows)."""
    if params.band_rows == 0 or params.n_parts <= 1:
        return list(range(height))
    return [y for y in range(height) if (y // params.band_rows) % params.n_parts == params.part]


class HostScene:
    """`(Camera, world, lights)` as loaded by the reference's main() (src/main.rs:26-59)."""

    def __init__(self, args: Sequence[str], cwd: Optional[str] = None):
        lib = load_host_lib()
        argv = [b"rtrace"] + [a.encode() for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        handle = C.c_void_p()
        old = os.getcwd()
        try:
            os.chdir(cwd or REPO_DIR)  # scene/asset paths are relative to the CWD, like the reference
            st = lib.rth_load(len(argv), arr, C.byref(handle))
        finally:
            os.chdir(old)
        _check(lib, st)
        self._lib = lib
        self._h = handle
        self.desc = lib.rth_scene(handle)          # POINTER(RtSceneDesc)
        self.camera = lib.rth_camera(handle).contents
        self.params = lib.rth_params(handle).contents.copy()
        self.gpus = lib.rth_gpus(handle)
        self.spp = lib.rth_samples_per_pixel(handle)
        self.log = lib.rth_log(handle).decode()
        xy = np.zeros((lib.rth_pick(handle, None, 0), 2), dtype=np.uint32)
        lib.rth_pick(handle, xy.ctypes.data, len(xy))
        self.pick = [(int(x), int(y)) for x, y in xy]  # --pick=<x>,<y>[:<x>,<y>...]: pixels to query instead of rendering
        dist = C.c_double()
        self.ao = (int(lib.rth_ao(handle, C.byref(dist))), dist.value)  # --ao=<samples>[:<max_distance>]: (0, inf) without the flag
        self.irradiance = bool(lib.rth_irradiance(handle))  # --irradiance: also bake out_irradiance.png
        self.sh_probes = np.zeros((lib.rth_sh_probes(handle, None, 0), 3))  # --sh-probe=<x>,<y>,<z>[:...]: (n, 3) positions to bake instead of rendering
        lib.rth_sh_probes(handle, self.sh_probes.ctypes.data, len(self.sh_probes))
        self.nearest = np.zeros((lib.rth_nearest_points(handle, None, 0), 3))  # --nearest=<x>,<y>,<z>[:...]: (n, 3) points to query instead of rendering
        lib.rth_nearest_points(handle, self.nearest.ctypes.data, len(self.nearest))
        pos = (C.c_double * 3)()
        width = int(lib.rth_probe(handle, pos))
        self.probe = (width, tuple(pos)) if width else None  # --probe=<x>,<y>,<z>[:<width>]: (width, position), None without the flag

    @property
    def width(self) -> int:
        return self.camera.image_width

    @property
    def height(self) -> int:
        return self.camera.image_height

    def close(self):
        if self._h:
            self._lib.rth_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tonemap_rgb8(rgba: np.ndarray) -> np.ndarray:
    """ACES + sRGB + 8-bit quantisation of an (H, W, 4) f64 frame -> (H, W, 3) uint8."""
    lib = load_host_lib()
    rgba = np.ascontiguousarray(rgba, dtype=np.float64)
    h, w = rgba.shape[:2]
    out = np.empty((h, w, 3), dtype=np.uint8)
    st = lib.rth_tonemap_rgb8(rgba.ctypes.data, w, h, out.ctypes.data)
    _check(lib, st)
    return out


def tonemap_rgb8_device(d_rgba: int, width: int, height: int, d_rgb: int, device: int = 0, stream: int = 0) -> None:
    """rt_tonemap_rgb8_device: tonemap_rgb8 on the GPU, device pointers in and out (width*height RGBA doubles ->
    width*height*3 bytes); returns when the output is written."""
    lib = load_device_lib()
    st = lib.rt_tonemap_rgb8_device(device, C.c_void_p(d_rgba), width, height, C.c_void_p(d_rgb), C.c_void_p(stream))
    _check(lib, st)


def _dp_ref(dp: Optional[RtDenoiseParams]):
    return C.byref(dp) if dp is not None else None


def denoise(rgba: np.ndarray, aov: np.ndarray, dp: Optional[RtDenoiseParams] = None, device: int = 0) -> np.ndarray:
    """rt_denoise: the (H, W, 4) f64 image filtered on the GPU, guided by its (H, W, 8) AOV image (DeviceScene.render_aov);
    dp None = the defaults."""
    lib = load_device_lib()
    rgba = np.ascontiguousarray(rgba, dtype=np.float64)
    aov = np.ascontiguousarray(aov, dtype=np.float64)
    h, w = rgba.shape[:2]
    if rgba.shape != (h, w, 4) or aov.shape != (h, w, AOV_CHANNELS):
        raise ValueError(f"denoise: expected (H, W, 4) and (H, W, {AOV_CHANNELS}) arrays, got {rgba.shape} and {aov.shape}")
    out = np.empty_like(rgba)
    st = lib.rt_denoise(device, rgba.ctypes.data, aov.ctypes.data, w, h, _dp_ref(dp), out.ctypes.data)
    _check(lib, st)
    return out


def denoise_device(d_rgba: int, d_aov: int, width: int, height: int, d_out: int, dp: Optional[RtDenoiseParams] = None,
                   device: int = 0, stream: int = 0) -> None:
    """rt_denoise_device: the same on device pointers (d_out may be d_rgba); returns when the output is written."""
    lib = load_device_lib()
    st = lib.rt_denoise_device(device, C.c_void_p(d_rgba), C.c_void_p(d_aov), width, height, _dp_ref(dp), C.c_void_p(d_out),
                               C.c_void_p(stream))
    _check(lib, st)


def probe_rays(position, width: int, height: int) -> tuple:
    """rth_probe_rays: the rays of an equirectangular light probe at `position` (+y up, row 0 at the top, the centre column
    looking along -z) as (origins, dirs), (width * height, 3) float64 each, row-major; DeviceScene.render_rays takes them."""
    lib = load_host_lib()
    o = np.empty((int(width) * int(height), 3), dtype=np.float64)
    d = np.empty_like(o)
    st = lib.rth_probe_rays((C.c_double * 3)(*[float(x) for x in position]), width, height, o.ctypes.data, d.ctypes.data)
    _check(lib, st)
    return o, d


def save_png(path: str, rgba: np.ndarray) -> None:
    lib = load_host_lib()
    rgba = np.ascontiguousarray(rgba, dtype=np.float64)
    h, w = rgba.shape[:2]
    st = lib.rth_save_png(path.encode(), rgba.ctypes.data, w, h)
    _check(lib, st)


def load_image(path: str) -> np.ndarray:
    """Buffer::from_image (buffer.rs:30-48): PNG / baseline JPEG -> (h, w, 3) float32."""
    lib = load_host_lib()
    ptr = C.POINTER(C.c_float)()
    w, h = C.c_uint32(), C.c_uint32()
    st = lib.rth_load_image(path.encode(), C.byref(ptr), C.byref(w), C.byref(h))
    _check(lib, st)
    try:
        return np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()
    finally:
        lib.rth_free_image(ptr)


SHADE_RAYS_STRIDE = 28  # RT_SHADE_RAYS_STRIDE


class DeviceScene:
    """RtScene on one GPU: the drop-in for `camera.render(world, lights, &mut buf)`."""

    def __init__(self, desc, device: int = 0):
        lib = load_device_lib()
        handle = C.c_void_p()
        st = lib.rt_scene_create(desc, device, C.byref(handle))
        _check(lib, st)
        self._lib = lib
        self._h = handle
        self.device = device

    def render(self, camera: RtCameraDesc, params: RtRenderParams) -> np.ndarray:
        rows = self._lib.rt_owned_rows(camera.image_height, C.byref(params))
        out = np.empty((rows, camera.image_width, 4), dtype=np.float64)
        st = self._lib.rt_render(self._h, C.byref(camera), C.byref(params), out.ctypes.data)
        _check(self._lib, st)
        return out

    def render_device(self, camera: RtCameraDesc, params: RtRenderParams, d_out_ptr: int, stream: int = 0) -> None:
        st = self._lib.rt_render_device(self._h, C.byref(camera), C.byref(params),
                                        C.c_void_p(d_out_ptr), C.c_void_p(stream))
        _check(self._lib, st)

    def render_light_groups(self, camera: RtCameraDesc, params: RtRenderParams, groups: RtLightGroups) -> tuple:
        """rt_render_light_groups: ((G, owned rows, W, 4) group frames, (owned rows, W, 4) ordinary frame) from one render."""
        rows = self._lib.rt_owned_rows(camera.image_height, C.byref(params))
        out_g = np.empty((groups.n_groups, rows, camera.image_width, 4), dtype=np.float64)
        out = np.empty((rows, camera.image_width, 4), dtype=np.float64)
        st = self._lib.rt_render_light_groups(self._h, C.byref(camera), C.byref(params), C.byref(groups), out_g.ctypes.data,
                                              out.ctypes.data)
        _check(self._lib, st)
        return out_g, out

    def render_light_groups_device(self, camera: RtCameraDesc, params: RtRenderParams, groups: RtLightGroups, d_groups_ptr: int,
                                   d_out_ptr: int = 0, stream: int = 0) -> None:
        st = self._lib.rt_render_light_groups_device(self._h, C.byref(camera), C.byref(params), C.byref(groups),
                                                     C.c_void_p(d_groups_ptr), C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def render_aov(self, camera: RtCameraDesc, params: RtRenderParams, n_replicas: Optional[int] = None) -> np.ndarray:
        """rt_render_aov: (owned rows, W, 8) first-hit albedo rgb, normal xyz, depth, coverage over the first n_replicas
        replicas (None = all thread_count of them)."""
        n = params.thread_count if n_replicas is None else n_replicas
        rows = self._lib.rt_owned_rows(camera.image_height, C.byref(params))
        out = np.empty((rows, camera.image_width, AOV_CHANNELS), dtype=np.float64)
        st = self._lib.rt_render_aov(self._h, C.byref(camera), C.byref(params), n, out.ctypes.data)
        _check(self._lib, st)
        return out

    def render_aov_device(self, camera: RtCameraDesc, params: RtRenderParams, d_out_ptr: int, n_replicas: Optional[int] = None,
                          stream: int = 0) -> None:
        n = params.thread_count if n_replicas is None else n_replicas
        st = self._lib.rt_render_aov_device(self._h, C.byref(camera), C.byref(params), n, C.c_void_p(d_out_ptr), C.c_void_p(stream))
        _check(self._lib, st)

    def trace_sample(self, camera, params, tid, x, y, sx, sy, max_bounces=64):
        """Diagnostic: (rgb[3], trace[n, 17]) of one sample traced on the device."""
        rgb = (C.c_double * 3)()
        tr = (C.c_double * (17 * max_bounces))()
        n = self._lib.rt_debug_trace_sample(self._h, C.byref(camera), C.byref(params), tid, x, y, sx, sy,
                                            rgb, tr, max_bounces)
        if n < 0:
            _check(self._lib, n)
        return np.array(list(rgb)), np.array(list(tr)).reshape(max_bounces, 17)[:min(n, max_bounces)]

    def shade_rays(self, params, origins, dirs, states, variant: int = 0) -> tuple:
        """rt_debug_shade_rays: one path vertex per ray on the device, (out[n, SHADE_RAYS_STRIDE], state_out[n]); variant 0 =
        the kernel variant the render picks, 1 = the full one, 2 = the simple one."""
        rays = np.ascontiguousarray(np.concatenate([np.asarray(origins, dtype=np.float64).reshape(-1, 3),
                                                    np.asarray(dirs, dtype=np.float64).reshape(-1, 3)], axis=1))
        st_in = np.ascontiguousarray(states, dtype=np.uint64)
        n = len(rays)
        if len(st_in) != n:
            raise ValueError("shade_rays: one generator state per ray")
        out = np.zeros((n, SHADE_RAYS_STRIDE), dtype=np.float64)
        st_out = np.zeros(n, dtype=np.uint64)
        st = self._lib.rt_debug_shade_rays(self._h, C.byref(params), variant, n, rays.ctypes.data, st_in.ctypes.data, out.ctypes.data,
                                           st_out.ctypes.data)
        _check(self._lib, st)
        return out, st_out

    def update(self, desc) -> dict:
        """rt_scene_update: gives the scene the numbers of `desc` (same structure: see include/rt_mi355.h); the mesh BVHs keep
        their trees and are refitted on the device.  Returns RtSceneUpdateInfo as a dict.  Accumulators (ProgressiveRender)
        created before raise the library's error from then on."""
        info = RtSceneUpdateInfo()
        st = self._lib.rt_scene_update(self._h, desc, C.byref(info))
        _check(self._lib, st)
        return {"n_meshes_refit": info.n_meshes_refit, "n_triangles_refit": info.n_triangles_refit, "bytes_uploaded": info.bytes_uploaded,
                "refit_kernel_ms": info.refit_kernel_ms, "total_ms": info.total_ms}

    def debug_mesh(self, mesh: int = 0, f32: bool = False) -> dict:
        """rt_debug_scene_mesh: what k_wf_mesh reads on the device for mesh instance `mesh`, in the form of
        api.scene_refit_mesh (the precision is materialised if needed)."""
        return _mesh_export(lambda *out: self._lib.rt_debug_scene_mesh(self._h, mesh, int(f32), *out))

    def debug_mesh_digest(self, f32: bool = False) -> tuple:
        """rt_debug_scene_mesh_digest: digests of the seven mesh tables on the device (BVH2 nodes, 4-wide f32 nodes, quantised
        nodes + cones, records, attributes, mesh boxes, mesh op records) and the number of updates so far."""
        out = (C.c_uint64 * 8)()
        st = self._lib.rt_debug_scene_mesh_digest(self._h, int(f32), out)
        _check(self._lib, st)
        return tuple(int(x) for x in out)

    @staticmethod
    def _rays(origins, dirs) -> tuple:
        """(n, 3) float64 C-contiguous origins and directions, broadcast against each other."""
        o, d = np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
        if o.shape[-1:] != (3,) or d.shape[-1:] != (3,):
            raise ValueError("origins and dirs must have a last axis of 3")
        o, d = np.broadcast_arrays(_table(o, "origins and dirs"), _table(d, "origins and dirs"))
        return np.ascontiguousarray(o), np.ascontiguousarray(d)

    def trace_rays(self, origins, dirs, precision: int = RT_PRECISION_F64) -> np.ndarray:
        """rt_trace_rays: the closest hit of every ray over (0.001, inf) as an (n,) array of api.RtRayHit.  origins / dirs:
        (n, 3) or (3,) (broadcast); directions need not be unit length."""
        o, d = self._rays(origins, dirs)
        out = np.zeros(len(o), dtype=RtRayHit)
        st = self._lib.rt_trace_rays(self._h, len(o), o.ctypes.data, d.ctypes.data, precision, out.ctypes.data)
        _check(self._lib, st)
        return out

    def trace_rays_device(self, n: int, d_origins_ptr: int, d_dirs_ptr: int, d_hits_ptr: int, precision: int = RT_PRECISION_F64,
                          stream: int = 0) -> None:
        """rt_trace_rays_device: n x 3 doubles each in HBM -> n RtRayHit records (96 B each) in HBM."""
        st = self._lib.rt_trace_rays_device(self._h, n, C.c_void_p(d_origins_ptr or None), C.c_void_p(d_dirs_ptr or None), precision,
                                            C.c_void_p(d_hits_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def occluded(self, origins, dirs, t_min=None, t_max=None, precision: int = RT_PRECISION_F64) -> np.ndarray:
        """rt_occluded: (n,) bool, True where a sphere, quad or triangle is hit inside (t_min, t_max).  t_min / t_max: None
        (0.001 / inf), a scalar or (n,)."""
        o, d = self._rays(origins, dirs)
        n = len(o)
        lo = None if t_min is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,)))
        hi = None if t_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=np.float64), (n,)))
        out = np.zeros(n, dtype=np.uint8)
        st = self._lib.rt_occluded(self._h, n, o.ctypes.data, d.ctypes.data, None if lo is None else lo.ctypes.data,
                                   None if hi is None else hi.ctypes.data, precision, out.ctypes.data)
        _check(self._lib, st)
        return out.astype(bool)

    def occluded_device(self, n: int, d_origins_ptr: int, d_dirs_ptr: int, d_out_ptr: int, d_t_min_ptr: int = 0, d_t_max_ptr: int = 0,
                        precision: int = RT_PRECISION_F64, stream: int = 0) -> None:
        """rt_occluded_device: n bytes (0 / 1) in HBM; d_t_min_ptr / d_t_max_ptr 0 = the defaults."""
        st = self._lib.rt_occluded_device(self._h, n, C.c_void_p(d_origins_ptr or None), C.c_void_p(d_dirs_ptr or None),
                                          C.c_void_p(d_t_min_ptr or None), C.c_void_p(d_t_max_ptr or None), precision,
                                          C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def render_rays(self, origins, dirs, params: RtRenderParams) -> np.ndarray:
        """rt_render_rays: the radiance along every ray as (n, 4) float64, (r, g, b, 0): ray i is rendered as pixel i of a frame
        whose camera sends every sample along it (sqrt_spt, thread_count, max_depth, background, light_bias, seed and precision
        of `params`).  origins / dirs: (n, 3) or (3,) (broadcast); directions need not be unit length."""
        o, d = self._rays(origins, dirs)
        out = np.empty((len(o), 4), dtype=np.float64)
        st = self._lib.rt_render_rays(self._h, len(o), o.ctypes.data, d.ctypes.data, C.byref(params), out.ctypes.data)
        _check(self._lib, st)
        return out

    def render_rays_device(self, n: int, d_origins_ptr: int, d_dirs_ptr: int, params: RtRenderParams, d_out_ptr: int,
                           stream: int = 0) -> None:
        """rt_render_rays_device: n x 3 doubles each in HBM -> n x 4 doubles in HBM."""
        st = self._lib.rt_render_rays_device(self._h, n, C.c_void_p(d_origins_ptr or None), C.c_void_p(d_dirs_ptr or None),
                                             C.byref(params), C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def bake_irradiance(self, positions, normals, params: RtRenderParams) -> np.ndarray:
        """rt_bake_irradiance: the cosine-weighted mean of the radiance arriving at every surface point as (n, 4) float64,
        (r, g, b, 0): S^2 x T paths per point from the full path tracer, their first directions drawn about the normal on the
        device (sqrt_spt, thread_count, max_depth, background, light_bias, seed and precision of `params`).  Irradiance is
        pi * out, a Lambertian texel's outgoing radiance albedo * out.  positions / normals: (n, 3) or (3,) (a single normal or
        position broadcasts); normals need not be unit length."""
        p, nr = self._rays(positions, normals)
        out = np.empty((len(p), 4), dtype=np.float64)
        st = self._lib.rt_bake_irradiance(self._h, len(p), p.ctypes.data, nr.ctypes.data, C.byref(params), out.ctypes.data)
        _check(self._lib, st)
        return out

    def bake_irradiance_device(self, n: int, d_positions_ptr: int, d_normals_ptr: int, params: RtRenderParams, d_out_ptr: int,
                               stream: int = 0) -> None:
        """rt_bake_irradiance_device: n x 3 doubles each in HBM -> n x 4 doubles in HBM."""
        st = self._lib.rt_bake_irradiance_device(self._h, n, C.c_void_p(d_positions_ptr or None), C.c_void_p(d_normals_ptr or None),
                                                 C.byref(params), C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def bake_irradiance_hits_device(self, n: int, d_hits_ptr: int, params: RtRenderParams, d_out_ptr: int, stream: int = 0) -> None:
        """rt_bake_irradiance_hits_device: n RtRayHit records in HBM (trace_rays_device) -> n x 4 doubles in HBM; a miss or an
        environment hit gives (0, 0, 0, 0)."""
        st = self._lib.rt_bake_irradiance_hits_device(self._h, n, C.c_void_p(d_hits_ptr or None), C.byref(params),
                                                      C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def bake_probes(self, positions, params: RtRenderParams) -> np.ndarray:
        """rt_bake_probes: SH radiance probes at positions in free space as (n, 9, 4) float64, (r, g, b, 0) per coefficient of
        the real L2 basis: the mean of L * Y_k over S^2 x T paths of the full path tracer per probe, their first directions
        uniform over the sphere and drawn on the device (sqrt_spt, thread_count, max_depth, background, light_bias, seed and
        precision of `params`).  The radiance coefficients are 4 pi * out; api.sh_irradiance lights a normal from them.
        positions: (n, 3) or (3,)."""
        p = _table(positions, "positions")
        out = np.empty((len(p), 9, 4), dtype=np.float64)
        st = self._lib.rt_bake_probes(self._h, len(p), p.ctypes.data, C.byref(params), out.ctypes.data)
        _check(self._lib, st)
        return out

    def bake_probes_device(self, n: int, d_positions_ptr: int, params: RtRenderParams, d_out_ptr: int, stream: int = 0) -> None:
        """rt_bake_probes_device: n x 3 doubles in HBM -> n x 9 x 4 doubles in HBM."""
        st = self._lib.rt_bake_probes_device(self._h, n, C.c_void_p(d_positions_ptr or None), C.byref(params), C.c_void_p(d_out_ptr or None),
                                             C.c_void_p(stream))
        _check(self._lib, st)

    @staticmethod
    def _points(points, max_distance) -> tuple:
        """(n, 3) float64 points and their (n,) limits (None: no limit; a scalar broadcasts)."""
        p = _table(points, "points")
        lim = None if max_distance is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_distance, dtype=np.float64), (len(p),)))
        return p, lim

    def closest_points(self, points, max_distance=None, precision: int = RT_PRECISION_F64) -> np.ndarray:
        """rt_closest_points: the nearest sphere, parallelogram or mesh triangle of the scene to every point as an (n,) array of
        api.RtPointHit (distance, closest point, geometric normal, ids, RT_POINT_* flags).  points: (n, 3) or (3,);
        max_distance: None (no limit), a scalar or (n,): a primitive counts only if it is strictly nearer."""
        p, lim = self._points(points, max_distance)
        out = np.zeros(len(p), dtype=RtPointHit)
        st = self._lib.rt_closest_points(self._h, len(p), p.ctypes.data, None if lim is None else lim.ctypes.data, precision, out.ctypes.data)
        _check(self._lib, st)
        return out

    def closest_points_device(self, n: int, d_points_ptr: int, d_out_ptr: int, d_max_distance_ptr: int = 0,
                              precision: int = RT_PRECISION_F64, stream: int = 0) -> None:
        """rt_closest_points_device: n x 3 doubles in HBM -> n RtPointHit records (80 B each) in HBM; d_max_distance_ptr 0 = no limit."""
        st = self._lib.rt_closest_points_device(self._h, n, C.c_void_p(d_points_ptr or None), C.c_void_p(d_max_distance_ptr or None), precision,
                                                C.c_void_p(d_out_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def point_query_stats(self) -> RtRayQueryStats:
        """rt_point_query_stats: of the last closest_points call (rays = points)."""
        s = RtRayQueryStats()
        st = self._lib.rt_point_query_stats(self._h, C.byref(s))
        _check(self._lib, st)
        return s

    def closest_points_counts(self, points, max_distance=None, precision: int = RT_PRECISION_F64) -> np.ndarray:
        """rt_debug_closest_points_counts: (n, 2) uint32, per point the BVH nodes visited and the triangles tested."""
        p, lim = self._points(points, max_distance)
        out = np.zeros((len(p), 2), dtype=np.uint32)
        st = self._lib.rt_debug_closest_points_counts(self._h, len(p), p.ctypes.data, None if lim is None else lim.ctypes.data, precision,
                                                      out.ctypes.data)
        _check(self._lib, st)
        return out

    def ray_query_stats(self) -> RtRayQueryStats:
        s = RtRayQueryStats()
        st = self._lib.rt_ray_query_stats(self._h, C.byref(s))
        _check(self._lib, st)
        return s

    def bake_visibility(self, positions, normals, samples: int = 64, seed: int = 0, bias: float = 1e-3,
                        max_distance: float = float("inf"), precision: int = RT_PRECISION_F64) -> np.ndarray:
        """rt_bake_visibility: ambient occlusion at surface points as an (n,) array of api.RtBakeResult: `visibility` = the
        share of `samples` cosine-weighted directions about the normal that are free over (bias, max_distance), `bent` = the
        sum of the free directions / samples.  positions / normals: (n, 3) or (3,) (a single normal broadcasts)."""
        p, nr = self._rays(positions, normals)
        out = np.zeros(len(p), dtype=RtBakeResult)
        bp = RtBakeParams.defaults(samples=samples, seed=seed, bias=bias, max_distance=max_distance, precision=precision)
        st = self._lib.rt_bake_visibility(self._h, len(p), p.ctypes.data, nr.ctypes.data, C.byref(bp), out.ctypes.data)
        _check(self._lib, st)
        return out

    def bake_visibility_device(self, n: int, d_positions_ptr: int, d_normals_ptr: int, d_out_ptr: int,
                               params: Optional[RtBakeParams] = None, stream: int = 0) -> None:
        """rt_bake_visibility_device: n x 3 doubles each in HBM -> n RtBakeResult records (32 B each) in HBM."""
        st = self._lib.rt_bake_visibility_device(self._h, n, C.c_void_p(d_positions_ptr or None), C.c_void_p(d_normals_ptr or None),
                                                 C.byref(params) if params is not None else None, C.c_void_p(d_out_ptr or None),
                                                 C.c_void_p(stream))
        _check(self._lib, st)

    def bake_visibility_hits_device(self, n: int, d_hits_ptr: int, d_out_ptr: int, params: Optional[RtBakeParams] = None,
                                    stream: int = 0) -> None:
        """rt_bake_visibility_hits_device: n RtRayHit records in HBM (trace_rays_device) -> n RtBakeResult records in HBM;
        a miss or an environment hit gives (1, 0, 0, 0)."""
        st = self._lib.rt_bake_visibility_hits_device(self._h, n, C.c_void_p(d_hits_ptr or None),
                                                      C.byref(params) if params is not None else None, C.c_void_p(d_out_ptr or None),
                                                      C.c_void_p(stream))
        _check(self._lib, st)

    def bake_stats(self) -> RtRayQueryStats:
        """rt_bake_stats: of the last bake (rays = n * samples); ray_query_stats() is not touched by a bake."""
        s = RtRayQueryStats()
        st = self._lib.rt_bake_stats(self._h, C.byref(s))
        _check(self._lib, st)
        return s

    def lightmap_texels(self, node: int, width: int, height: int, instance: int = 0, counts: bool = False):
        """rt_lightmap_texels: the UV atlas of mesh node `node` (RtSceneDesc.nodes index; `instance`: the k-th op of the program
        that came from it) rasterised into (height, width) api.RtRayHit records, row 0 = v near 0; an uncovered texel holds the
        miss record.  counts=True: also the (height, width) uint32 number of triangles that cover each texel centre."""
        ok = 0 < width <= 16384 and 0 < height <= 16384
        hits = np.zeros((height, width) if ok else (1, 1), dtype=RtRayHit)
        cnt = np.zeros(hits.shape, dtype=np.uint32) if counts else None
        st = self._lib.rt_lightmap_texels(self._h, node, instance, width, height, hits.ctypes.data, None if cnt is None else cnt.ctypes.data)
        _check(self._lib, st)
        return (hits, cnt) if counts else hits

    def lightmap_texels_device(self, node: int, width: int, height: int, d_hits_ptr: int, d_counts_ptr: int = 0, instance: int = 0,
                               stream: int = 0) -> None:
        """rt_lightmap_texels_device: width * height RtRayHit records (96 B each) into HBM; d_counts_ptr 0 = no counts."""
        st = self._lib.rt_lightmap_texels_device(self._h, node, instance, width, height, C.c_void_p(d_hits_ptr or None),
                                                 C.c_void_p(d_counts_ptr or None), C.c_void_p(stream))
        _check(self._lib, st)

    def bake_lightmap(self, node: int, width: int, height: int, params, kind: str = "irradiance", dilate: int = 2, instance: int = 0) -> tuple:
        """rt_bake_lightmap: rasterise, bake and dilate in one call, everything on the device in between -> ((height, width, 4)
        float64 image, (height, width) uint8 coverage before dilation).  kind "irradiance": params is an RtRenderParams
        (rt_bake_irradiance's conventions); kind "visibility": params is an RtBakeParams or None (its defaults)."""
        k = _LIGHTMAP_KINDS[kind] if isinstance(kind, str) else int(kind)
        ok = 0 < width <= 16384 and 0 < height <= 16384
        out = np.zeros((height, width, 4) if ok else (1, 1, 4), dtype=np.float64)
        cov = np.zeros(out.shape[:2], dtype=np.uint8)
        rp = C.byref(params) if isinstance(params, RtRenderParams) else None
        bp = C.byref(params) if isinstance(params, RtBakeParams) else None
        st = self._lib.rt_bake_lightmap(self._h, node, instance, width, height, k, rp, bp, dilate, out.ctypes.data, cov.ctypes.data)
        _check(self._lib, st)
        return out, cov

    def lightmap_stats(self) -> RtLightmapStats:
        """rt_lightmap_stats: HIP-event times of the last rasterisation (binning, raster), covered texels, tile references."""
        s = RtLightmapStats()
        st = self._lib.rt_lightmap_stats(self._h, C.byref(s))
        _check(self._lib, st)
        return s

    def stats(self) -> RtRenderStats:
        s = RtRenderStats()
        st = self._lib.rt_get_stats(self._h, C.byref(s))
        _check(self._lib, st)
        return s

    def close(self):
        if self._h:
            self._lib.rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveRender:
    """A frame rendered in passes of replicas (rt_accum_*, include/rt_mi355.h): after every pass `estimate()` is the
    frame's expected value from the replicas so far, and once all `thread_count` replicas are done it IS the frame
    DeviceScene.render returns, bit for bit, however the passes were split.  `save_state()` / `load_state()` carry the
    sums to another process (same scene description, camera and params).

    `adaptive` (RtAdaptiveParams) opts into adaptive sampling (rt_accum_set_adaptive): pixels whose noise estimate, and
    that of their neighbourhood, has fallen below the threshold stop receiving replicas; `sample_counts()` tells how
    many each pixel got and `estimate()` scales every pixel by its own count."""

    def __init__(self, scene: DeviceScene, camera: RtCameraDesc, params: RtRenderParams,
                 adaptive: Optional[RtAdaptiveParams] = None):
        lib = load_device_lib()
        handle = C.c_void_p()
        st = lib.rt_accum_create(scene._h, C.byref(camera), C.byref(params), C.byref(handle))
        _check(lib, st)
        self._lib = lib
        self._h = handle
        self.scene = scene  # the device scene must outlive the accumulator
        self.camera = camera
        self.params = params.copy()
        self.rows = lib.rt_owned_rows(camera.image_height, C.byref(params))
        self.total = params.thread_count
        self.adaptive = None
        if adaptive is not None:
            st = lib.rt_accum_set_adaptive(handle, C.byref(adaptive))
            try:
                _check(lib, st)
            except RtError:
                self.close()
                raise
            self.adaptive = RtAdaptiveParams.from_buffer_copy(adaptive)

    def _check(self, st: int) -> None:
        _check(self._lib, st)

    def render(self, n: int, pipeline: Optional[int] = None, collect_stats: Optional[bool] = None) -> int:
        """Renders the next n replicas (clamped to what is left); returns replicas_done."""
        p = None
        if pipeline is not None or collect_stats is not None:
            p = self.params.copy()
            if pipeline is not None:
                p.pipeline = pipeline
            if collect_stats is not None:
                p.collect_stats = int(bool(collect_stats))
        self._check(self._lib.rt_accum_render(self._h, n, C.byref(p) if p is not None else None, None))
        return self.replicas_done

    @property
    def replicas_done(self) -> int:
        return int(self._lib.rt_accum_replicas_done(self._h))

    @property
    def active_pixels(self) -> int:
        """Pixels that still receive replicas (0 once the frame is finished)."""
        return int(self._lib.rt_accum_active_pixels(self._h))

    @property
    def finished(self) -> bool:
        """All replicas done, or (adaptive) every pixel has stopped: render() renders nothing any more."""
        return bool(self._lib.rt_accum_finished(self._h))

    def sample_counts(self) -> np.ndarray:
        """Replicas in each pixel's sum (uint32, rows x width)."""
        out = np.empty((self.rows, self.camera.image_width), dtype=np.uint32)
        self._check(self._lib.rt_accum_sample_counts(self._h, out.ctypes.data))
        return out

    def noise(self) -> np.ndarray:
        """Relative standard error of each pixel's luminance at its replica count (adaptive accumulators only)."""
        out = np.empty((self.rows, self.camera.image_width), dtype=np.float64)
        self._check(self._lib.rt_accum_noise(self._h, out.ctypes.data))
        return out

    def estimate(self) -> np.ndarray:
        out = np.empty((self.rows, self.camera.image_width, 4), dtype=np.float64)
        self._check(self._lib.rt_accum_estimate(self._h, out.ctypes.data))
        return out

    def estimate_device(self, d_out_ptr: int, stream: int = 0) -> None:
        self._check(self._lib.rt_accum_estimate_device(self._h, C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def preview_rgb8(self) -> np.ndarray:
        out = np.empty((self.rows, self.camera.image_width, 3), dtype=np.uint8)
        self._check(self._lib.rt_accum_preview_rgb8(self._h, out.ctypes.data))
        return out

    def estimate_denoised(self, dp: Optional[RtDenoiseParams] = None) -> np.ndarray:
        """The estimate through rt_denoise, guided by AOVs the accumulator renders on first use (dp.aov_replicas)."""
        out = np.empty((self.rows, self.camera.image_width, 4), dtype=np.float64)
        self._check(self._lib.rt_accum_estimate_denoised(self._h, _dp_ref(dp), out.ctypes.data))
        return out

    def preview_rgb8_denoised(self, dp: Optional[RtDenoiseParams] = None) -> np.ndarray:
        out = np.empty((self.rows, self.camera.image_width, 3), dtype=np.uint8)
        self._check(self._lib.rt_accum_preview_denoised_rgb8(self._h, _dp_ref(dp), out.ctypes.data))
        return out

    def save_state(self) -> bytes:
        n = self._lib.rt_accum_state_size(self._h)
        buf = C.create_string_buffer(n)
        self._check(self._lib.rt_accum_save_state(self._h, buf, n))
        return buf.raw

    def load_state(self, blob: bytes) -> None:
        self._check(self._lib.rt_accum_load_state(self._h, blob, len(blob)))

    def close(self):
        if self._h:
            self._lib.rt_accum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FramePipeline:
    """A sequence of frames of one scene on one GPU with their tails overlapped (rt_scene_set_tail_flag, include/rt_mi355.h).

    The end of a render is a chain of small, latency-bound launches (the last, longest paths: 20 of the 44 iterations of a
    1/8-frame share, 10 % of its time) that no scheduling inside ONE frame can fill.  Here `depth` device scenes of the
    same description are driven by one host thread each, on one stream each; frame k starts when frame k-1 reports that
    it has entered its tail, so its full launches run underneath.  Every frame is the frame DeviceScene.render_device
    produces on its own (same kernels, same per-sample RNG keys): tests/test_gpu_parity.py::test_frame_pipeline_*.
    """

    def __init__(self, desc, device: int = 0, depth: int = 2, scenes=None):
        """`scenes`: ready-made device scenes instead of `depth` new ones (the CPU tests of the ordering logic pass stand-ins)."""
        self.scenes = list(scenes) if scenes is not None else [DeviceScene(desc, device) for _ in range(max(1, depth))]
        self.device = device

    @property
    def depth(self) -> int:
        return len(self.scenes)

    def render_frames(self, camera: RtCameraDesc, params_list, d_out_ptrs, streams):
        """Frame k: params_list[k] into device buffer d_out_ptrs[k]; streams: one raw stream handle per device scene (all
        different, none the NULL stream).  Blocks until every frame is rendered; returns one RtRenderStats per frame."""
        import threading
        import time
        n, depth = len(params_list), len(self.scenes)
        if len(d_out_ptrs) != n or len(streams) < depth:
            raise ValueError("render_frames: one output buffer per frame and one stream per device scene")
        flags = (C.c_int32 * max(n, 1))()  # flags[k]: frame k has entered its tail (or returned)
        log = os.environ.get("RT_PIPE_LOG", "0") == "1"
        t_origin = time.perf_counter()
        stats = [None] * n
        errors = []

        def worker(i):
            sc = self.scenes[i]
            lib = sc._lib
            k = i
            try:
                while k < n:
                    if k > 0:
                        while flags[k - 1] == 0 and not errors:
                            time.sleep(0.0002)
                    if errors:
                        break
                    lib.rt_scene_set_tail_flag(sc._h, C.addressof(flags) + 4 * k)
                    t_start = time.perf_counter()
                    sc.render_device(camera, params_list[k], d_out_ptrs[k], streams[i])
                    stats[k] = sc.stats()
                    if log:
                        sys.stderr.write(f"[frame pipeline] frame {k} on scene {i}: start {1e3 * (t_start - t_origin):.1f} ms, "
                                         f"end {1e3 * (time.perf_counter() - t_origin):.1f} ms, kernels {stats[k].kernel_ms:.1f} ms\n")
                    k += depth
            except Exception as e:  # noqa: BLE001 - reported to the caller below
                errors.append(e)
            finally:
                for j in range(k, n, depth):  # frames this thread will not render: nobody may wait for them
                    flags[j] = 1
                lib.rt_scene_set_tail_flag(sc._h, None)

        threads = [threading.Thread(target=worker, args=(i,), name=f"rt-frame-{i}") for i in range(min(depth, n))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        return stats

    def close(self):
        for sc in self.scenes:
            sc.close()

