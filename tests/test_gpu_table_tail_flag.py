"""The tail flag (rt_scene_set_tail_flag) and the seven entry points of the table modes: rt_render_rays, rt_bake_irradiance and
rt_bake_probes with their device variants.  Each releases whoever waits for the render's tail at the latest when it returns, a
call that is refused included, and a refused call leaves its output alone.  Eight rays of render_rays_ref's cornell case, one
path each: one chunk, one replica group."""
import ctypes as C

import numpy as np
import pytest

import render_rays_ref as rr
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

N = 8
ENTRY_POINTS = ("rt_render_rays", "rt_render_rays_device", "rt_bake_irradiance", "rt_bake_irradiance_device",
                "rt_bake_irradiance_hits_device", "rt_bake_probes", "rt_bake_probes_device")


def test_every_table_entry_point_raises_the_tail_flag_also_when_it_refuses():
    import torch
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    c = rr.case("cornell")
    o, d = np.ascontiguousarray(c.o[:N]), np.ascontiguousarray(c.d[:N])   # also positions and normals: d lies in the surface's hemisphere
    good = rr.params_for(c.hs, 1, 1, rr.SEED)
    bad = good.copy()
    bad.sqrt_spt = 0
    live0 = api.live_resources()
    scene = api.DeviceScene(c.hs.desc, 0)
    h = scene._h
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_hits = torch.zeros(N * api.RtRayHit.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.trace_rays_device(N, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr())   # the records of the same eight rays
    vp = lambda t: C.c_void_p(t.data_ptr())

    def call(name, p, out, d_out):
        """One call of entry point `name`: the host variants write `out`, the device variants `d_out`."""
        pp, po, pd = C.byref(p), o.ctypes.data, d.ctypes.data
        if name == "rt_render_rays":
            return lib.rt_render_rays(h, N, po, pd, pp, out.ctypes.data)
        if name == "rt_render_rays_device":
            return lib.rt_render_rays_device(h, N, vp(d_o), vp(d_d), pp, vp(d_out), None)
        if name == "rt_bake_irradiance":
            return lib.rt_bake_irradiance(h, N, po, pd, pp, out.ctypes.data)
        if name == "rt_bake_irradiance_device":
            return lib.rt_bake_irradiance_device(h, N, vp(d_o), vp(d_d), pp, vp(d_out), None)
        if name == "rt_bake_irradiance_hits_device":
            return lib.rt_bake_irradiance_hits_device(h, N, vp(d_hits), pp, vp(d_out), None)
        if name == "rt_bake_probes":
            return lib.rt_bake_probes(h, N, po, pp, out.ctypes.data)
        assert name == "rt_bake_probes_device"
        return lib.rt_bake_probes_device(h, N, vp(d_o), pp, vp(d_out), None)

    flag = C.c_int32(0)
    assert lib.rt_scene_set_tail_flag(h, C.addressof(flag)) == api.RT_OK
    try:
        for name in ENTRY_POINTS:
            per_entry = 36 if "probes" in name else 4
            out = np.full((N, per_entry), 7.0)
            d_out = torch.full((N, per_entry), 7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            flag.value = 0
            st = call(name, bad, out, d_out)
            assert st == api.RT_E_INVALID, (name, st, lib.rt_last_error().decode())
            assert flag.value == 1, f"{name}: a refused call does not release the tail flag"
            assert (out == 7.0).all() and bool((d_out == 7.0).all()), f"{name}: a refused call wrote to its output"
            flag.value = 0
            st = call(name, good, out, d_out)
            assert st == api.RT_OK, (name, st, lib.rt_last_error().decode())
            assert flag.value == 1, f"{name}: a call that succeeds does not release the tail flag"
    finally:
        assert lib.rt_scene_set_tail_flag(h, None) == api.RT_OK
    scene.close()
    assert api.live_resources() == live0
