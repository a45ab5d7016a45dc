"""Ray queries, the parts that need no device: the op -> node table of the scene compiler (api.scene_op_nodes), the --pick
flag of the scene loader, the layout of api.RtRayHit and the guards of the shared ray sets (tests/ray_query_cases.py)."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import SCENES, WIDTHS, cases, host_scene, leaf_nodes

# rt_scene.h OpType
OP_SPHERE, OP_PLANE, OP_MESH, OP_SKY, OP_SUN, OP_VOL_END = 4, 5, 6, 7, 8, 11
NODE_OF_OP = {OP_SPHERE: api.RT_NODE_SPHERE, OP_PLANE: api.RT_NODE_PLANE, OP_MESH: api.RT_NODE_MESH, OP_SKY: api.RT_NODE_SKY,
              OP_SUN: api.RT_NODE_SUN}


def test_ray_hit_dtype_layout():
    dt = api.RtRayHit
    assert dt.itemsize == 96
    assert [dt.fields[f][1] for f in ("t", "pos", "normal", "u", "v", "material", "node", "prim", "flags", "_reserved")] == \
        [0, 8, 32, 56, 64, 72, 76, 80, 84, 88]
    assert (api.RT_RAY_HIT, api.RT_RAY_FRONT_FACE, api.RT_RAY_ENVIRONMENT) == (1, 2, 4)


@pytest.mark.parametrize("name", ["cornell", "two_meshes", "sphere_field", "nested_transform"])
def test_scene_op_nodes(name):
    hs = host_scene(name)
    d = hs.desc.contents
    ops, info = api.scene_program(hs.desc)
    nodes = api.scene_op_nodes(hs.desc)
    assert nodes.dtype == np.int32 and len(nodes) == len(ops)
    if name == "sphere_field":
        assert info["groups"] >= 1   # a rebuilt group: its ops are emitted by another routine
    seen = set()
    for (op, _arg, _skip, _chain), n in zip(ops, nodes):
        if op in NODE_OF_OP:
            assert 0 <= n < d.n_nodes and d.nodes[n].type == NODE_OF_OP[op]
            seen.add(int(n))
        else:
            assert n == -1
    assert seen == set(leaf_nodes(hs.desc)), "every reachable primitive node has an op, and no other node has one"
    if name == "two_meshes":
        meshes = [n for n in seen if d.nodes[n].type == api.RT_NODE_MESH]
        assert len(meshes) == 2


def test_pick_flag():
    assert api.HostScene([SCENES["cornell"], "-w=24"]).pick == []
    assert api.HostScene([SCENES["cornell"], "-w=24", "--pick=3,4"]).pick == [(3, 4)]
    hs = api.HostScene([SCENES["cornell"], "-w=24", "--pick=0,0:23,0:5,7"])
    assert hs.pick == [(0, 0), (23, 0), (5, 7)]
    assert hs.height > 7
    last = api.HostScene([SCENES["cornell"], "-w=24", f"--pick=23,{hs.height - 1}"])
    assert last.pick == [(23, hs.height - 1)]


@pytest.mark.parametrize("value", ["3", "3,", ",4", "3,4:", ":3,4", "3,4,5", "a,b", "-1,2", "1.5,2", "3;4", "3,4:5"])
def test_pick_flag_malformed(value):
    with pytest.raises(api.RtError) as e:
        api.HostScene([SCENES["cornell"], "-w=24", f"--pick={value}"])
    assert e.value.status == api.RT_E_INVALID and "Pick" in str(e.value)


@pytest.mark.parametrize("value", ["24,0", "0,1000", "3,4:24,4"])
def test_pick_flag_out_of_frame(value):
    with pytest.raises(api.RtError) as e:
        api.HostScene([SCENES["cornell"], "-w=24", f"--pick={value}"])
    assert e.value.status == api.RT_E_INVALID and "outside" in str(e.value)


def test_ray_sets_are_not_vacuous():
    """The shared recipe on its cheapest scene: sizes and the oracle-side guards every GPU test asserts."""
    c = cases("cornell")
    w = WIDTHS.get("cornell", 24)
    assert len(c.cam_o) == w * c.hs.height and len(c.fu_o) == len(c.P) and 0 < len(c.seg_o) <= len(c.P)
    c.assert_not_vacuous()
