"""The fixture of tests/tree_scale_cases.py and its tree checker on the host's own tables: the mesh at 131 072 triangles, its
three deformations, check_tree on the refit of the CPU (api.scene_refit_mesh) in both precisions, three mutants that
check_tree must refuse, and the ray sets' conditions on the oracle's answers.  No GPU."""
import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api
import tree_scale_cases as tc

CASES = ("base",) + tc.DEFORMATIONS


def export(case, f32):
    a, b = tc.host_scene("base"), tc.host_scene(case)
    return api.scene_refit_mesh(a.desc, b.desc, 0, f32)


def checked(t):
    return tc.check_tree(t["children"], t["boxes"], t["tris"], t["order"], tc.N_TRIS)


def test_fixture_sizes():
    hs = tc.host_scene("base")
    m = hs.desc.contents.meshes[0]
    assert hs.desc.contents.n_meshes == 1 and m.n_triangles == tc.N_TRIS == 131072 and m.n_positions == tc.N_POS == 65536
    st = api.scene_mesh_stats(hs.desc)
    print(st)
    assert st["triangles"] == tc.N_TRIS and st["bvh4_nodes"] >= 8192 and st["bvh4_stack"] > 12
    assert tc.worst_stack(export("base", False)["children"]) == st["bvh4_stack"]   # the figure read off an exported tree


def test_deformations():
    base = tc.positions(tc.host_scene("base"))
    assert tc.zero_area_triangles(tc.host_scene("base")) == 0
    assert tc.zero_area_triangles(tc.host_scene("weld")) == 2048
    assert (tc.positions(tc.host_scene("smooth")) != base).any(axis=1).all()        # every vertex moves
    assert int((tc.positions(tc.host_scene("weld")) != base).any(axis=1).sum()) == 1024
    ext = np.ptp(tc.positions(tc.host_scene("stretch")), axis=0)
    print("stretch extents", ext)
    assert ext[0] / ext[1] >= 1000
    for case in tc.DEFORMATIONS:
        for args in (tc.FRAME_ARGS, tc.RAY_ARGS):
            api.scene_update_check(tc.host_scene("base", args).desc, tc.host_scene(case, args).desc)
        assert np.isfinite(tc.positions(tc.host_scene(case))).all()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES)
def test_check_tree_accepts_the_hosts_tables(case, f32):
    slack = checked(export(case, f32))
    print(f"{case} {'f32' if f32 else 'f64'}: largest slack {slack:.3g} object units")
    assert slack >= 0


def test_check_tree_refuses_mutants():
    t = export("base", False)
    children, boxes, tris = t["children"], t["boxes"], t["tris"]
    lo, hi, _, _, _ = tc.tree_extents(children, tris, tc.N_TRIS)
    # 1. one child box shrunk by one quantisation cell on one axis: the upper x face of the child that fits tightest in its cell
    full = children != tc.EMPTY
    cells = np.array([tc.cell_of(boxes, i, 0) for i in range(len(children))])
    room = np.where(full, (boxes[:, :, 1, 0].astype(np.float64) - hi[:, :, 0]) / cells[:, None], np.inf)
    i, k = np.unravel_index(np.argmin(room), room.shape)
    assert 0 <= room[i, k] < 1
    shrunk = boxes.copy()
    shrunk[i, k, 1, 0] -= np.float32(cells[i])
    assert shrunk[i, k, 1, 0] < boxes[i, k, 1, 0] and shrunk[i, k, 0, 0] <= shrunk[i, k, 1, 0]
    with pytest.raises(AssertionError, match=rf"\(c\) node {i} child {k} axis 0"):
        tc.check_tree(children, shrunk, tris, t["order"], tc.N_TRIS)
    # 2. one leaf's count raised by one: a slot is covered twice
    leaves = np.argwhere((children < 0) & full & ((~children & 7) < 7) & ((~children >> 3) + (~children & 7) + 1 < tc.N_TRIS))
    i, k = leaves[len(leaves) // 2]
    longer = children.copy()
    longer[i, k] = ~(~children[i, k] + 1)
    with pytest.raises(AssertionError, match=r"\(b\) slot \d+ is covered 2 times"):
        tc.check_tree(longer, boxes, tris, t["order"], tc.N_TRIS)
    # 3. one inner child replaced by the empty marker: its slots are uncovered
    inner = np.argwhere(children >= 0)
    i, k = inner[len(inner) // 2]
    cut = children.copy()
    cut[i, k] = tc.EMPTY
    with pytest.raises(AssertionError):
        tc.check_tree(cut, boxes, tris, t["order"], tc.N_TRIS)
    cut_boxes = boxes.copy()   # the same with the box inverted as an empty child's is and the orphaned subtree's nodes left in place
    cut_boxes[i, k, 0], cut_boxes[i, k, 1] = np.inf, -np.inf
    with pytest.raises(AssertionError, match=r"\(a\)|\(b\)"):
        tc.check_tree(cut, cut_boxes, tris, t["order"], tc.N_TRIS)
    assert tc.check_tree(children, boxes, tris, t["order"], tc.N_TRIS) >= 0   # the originals still pass


@pytest.mark.parametrize("case", ["base", "smooth", "weld"])
def test_ray_sets_are_not_vacuous(case):
    r = tc.ray_sets(case)
    print(f"{case}: {len(r.cam_o)} camera rays, {r.mesh_share(r.cam_hits):.1%} on the mesh, {len(r.fu_o)} follow-ups "
          f"({r.mesh_share(r.fu_hits):.1%}), {len(r.aim_o)} aimed rays ({r.mesh_share(r.aim_hits):.1%}), {len(r.seg_o)} segments, "
          f"{r.seg_occluded.mean():.1%} occluded")
    assert len(r.cam_o) == 2304
    r.assert_not_vacuous()
    # the interval of a segment handed to the oracle itself gives the same flags
    seg, _ = pyoracle.world_hits(r.hs.desc, r.seg_o, r.seg_d, tc.T_MIN, tc.T_MAX)
    np.testing.assert_array_equal(seg[:, 10] >= 0, r.seg_occluded)
