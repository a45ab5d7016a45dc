"""The upload against the derivation: the seven mesh tables as they stand on the device after DeviceScene<R>::build equal,
byte for byte (by digest), the tables the host derives for the same description (rt_tables.cpp, api.scene_tables_digest).
One mesh; two meshes (the same file twice, and two files with different pads); a mesh under a transform chain of length 1,
where MeshOpRec::inv is filled.  The tables after an rt_scene_update are held to the host's in tests/test_gpu_scene_update.py."""
import pytest

from rust_raytracer_amd import api
from test_scene_tables_host import SCENES

pytestmark = pytest.mark.gpu

SCENES = dict(SCENES, nested_transform=lambda tmp_path: api.HostScene(["tests/scenes/nested_transform", "-w=8", "-s=1"]))
NAMES = ("BvhNode", "BvhNode4f", "MeshNode4qc", "TriRec", "TriAttr", "mesh_bounds", "MeshOpRec")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_uploaded_tables_are_the_derived_ones(tmp_path, name, f32):
    assert api.load_device_lib().rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    hs = SCENES[name](tmp_path)
    p = hs.params.copy()
    p.precision = api.RT_PRECISION_F32 if f32 else api.RT_PRECISION_F64
    scene = api.DeviceScene(hs.desc, 0)
    try:
        frame = scene.render(hs.camera, p)      # one 8 x 8 frame at 1 sample: the tables of this precision are on the device
        assert frame.shape[:2] == (8, 8)
        on_device = scene.debug_mesh_digest(f32)[:7]
    finally:
        scene.close()
    assert dict(zip(NAMES, on_device)) == dict(zip(NAMES, api.scene_tables_digest(hs.desc, f32)[:7]))
