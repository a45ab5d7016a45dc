"""The generated group scenes of tests/group_cases.py without a GPU: every scene sits on its intended side of each limit of
plan_wavefront, the group BVHs that k_wf_prims reads (api.scene_groups: compile_scene + derive_scene_tables, the derivation that
fills the device) are whole and stay inside their own ranges, and the ray sets reach every primitive (conditions on the oracle's
answers alone)."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import SURFACE
import group_cases as gc

OP_BOUNDS, OP_SPHERE, OP_PLANE, OP_GROUP = 1, 4, 5, 12
EMPTY = -2 ** 31
MAX_LEVELS, MAX_NODES = 16, 384          # plan_wavefront: 16 stack levels, 24 KB of 64-byte nodes
# what each scene is for: groups, primitives in them, and the side of each limit (None: not what the scene is about)
PLAN = {
    "two_groups": dict(groups=2, prims=74, bvh=True),        # 40 + (30 + 2 of the hollow ball + 2 quads); `lost` is dropped
    "two_groups_swapped": dict(groups=2, prims=74, bvh=True),
    "instanced": dict(groups=3, prims=100, bvh=True),
    "stack16": dict(groups=1, prims=gc.CHAIN3_AT, stack=(16, 16), bvh=True),
    "stack_over": dict(groups=1, prims=gc.CHAIN3_OVER, stack=(17, 99), bvh=False),
    "chain15_16": dict(groups=1, prims=gc.CHAIN15_AT, stack=(16, 16), bvh=True),
    "lattice900": dict(groups=1, prims=900, stack=(1, 16), bvh=True),
    "lattice1000": dict(groups=1, prims=1000, stack=(17, 99), bvh=False),
    "nodes_at_limit": dict(groups=2, prims=1536 + gc.SECOND_AT, stack=(1, 16), nodes=(380, 384), bvh=True),
    "nodes_over": dict(groups=2, prims=1536 + gc.SECOND_OVER, stack=(1, 16), nodes=(385, 400), bvh=False),
    "ground": dict(groups=1, prims=61, bvh=True),
    "far": dict(groups=1, prims=40, bvh=True),
}


def test_every_scene_is_listed():
    assert set(PLAN) == set(gc.NAMES) == set(gc.GROUP_FORM) | set(gc.OP_FORM)
    assert {n for n, p in PLAN.items() if p["bvh"]} == set(gc.GROUP_FORM)


@pytest.mark.parametrize("name", gc.NAMES)
def test_plan(name):
    _, info = gc.program(name)
    want = PLAN[name]
    print(name, {k: info[k] for k in ("groups", "group_nodes", "group_stack", "group_prims", "group_bvh")})
    assert info["groups"] == want["groups"] and info["group_prims"] == want["prims"]
    assert info["split"] and info["mesh_ops"] == 0 and info["volumes"] == 0
    lo, hi = want.get("stack", (1, MAX_LEVELS))
    assert lo <= info["group_stack"] <= hi
    lo, hi = want.get("nodes", (1, MAX_NODES))
    assert lo <= info["group_nodes"] <= hi
    assert info["group_bvh"] == want["bvh"]
    # the plan's rule itself
    assert info["group_bvh"] == (info["group_stack"] <= MAX_LEVELS and info["group_nodes"] <= MAX_NODES)


def test_the_chains_are_the_shortest():
    """stack_over is one sphere longer than stack16, so it is the shortest chain over the limit; a chain of ratio 1.5 one
    sphere shorter than chain15_16 needs fewer than 16 levels."""
    assert gc.CHAIN3_OVER == gc.CHAIN3_AT + 1
    text, _, _ = gc._chain(1.5, gc.CHAIN15_AT - 1)
    path = gc._tmp() / "scene_chain15_short"
    path.write_text(gc.MATERIALS + text + gc._tail("$chain", (0, 1e6, 0), 1))
    hs = api.HostScene([str(path), "-w=8", "-s=1"])
    _, info = api.scene_program(hs.desc)
    assert info["groups"] == 1 and info["group_stack"] == 15


def test_lds_of_the_limit_scenes():
    """lattice900's stack and nodes alone exceed the 44 KB above which make_search_setup leaves the small tables in global memory;
    nodes_at_limit asks for the largest launch the plan admits: 16 levels x 2048 B, 384 nodes x 64 B and the 8208 B of the mesh list."""
    _, info = gc.program("lattice900")
    assert info["group_stack"] * 2048 + info["group_nodes"] * 64 > 44 * 1024
    _, info = gc.program("nodes_at_limit")
    print("nodes_at_limit:", info["group_stack"] * 2048 + info["group_nodes"] * 64 + 8208, "B of dynamic LDS at most")
    assert info["group_stack"] * 2048 + info["group_nodes"] * 64 + 8208 == 65552


def _prim_box(desc, node):
    n = desc.contents.nodes[node]
    if n.type == api.RT_NODE_SPHERE:
        c, r = np.array(list(n.p)[:3]), abs(n.p[3])
        return c - r, c + r
    return np.array(list(n.bounds)[:3]), np.array(list(n.bounds)[3:6])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", gc.NAMES)
def test_tree(name, f32):
    hs = gc.host_scene(name)
    desc = hs.desc
    nodes = desc.contents.nodes
    ops, info = gc.program(name)
    op_nodes = api.scene_op_nodes(desc)
    g = api.scene_groups(desc, f32)
    g64 = g if not f32 else api.scene_groups(desc, False)
    children, boxes, prims, roots = g["children"], g["boxes"], g["prims"], g["roots"]
    assert len(roots) == info["groups"] and len(children) == info["group_nodes"] and len(prims) == info["group_prims"]
    # the bound is Collapser::max_stack: the entries a search can hold (below) and one spare level
    assert g["stack_levels"] == info["group_stack"]
    group_ops = np.flatnonzero(ops[:, 0] == OP_GROUP)
    assert len(group_ops) == len(roots) and (ops[group_ops, 1] == np.arange(len(roots))).all()
    assert roots[0] == 0 and (np.diff(roots.astype(np.int64)) > 0).all()
    prim_base, worst = 0, 0
    for gi, root in enumerate(roots):
        n_lo, n_hi = int(root), int(roots[gi + 1]) if gi + 1 < len(roots) else len(children)
        S = float(np.abs(g64["group_boxes"][gi]).max())
        pad = S / 524288.0                                     # 2^-19 x the largest |coordinate| of the group's box
        seen_nodes, positions = [], []

        def walk(node, held):
            """Returns the box of the primitives below; held = entries on the stack when the search stands at this node."""
            nonlocal worst
            assert n_lo <= node < n_hi, f"group {gi}: inner reference {node} outside its nodes [{n_lo}, {n_hi})"
            seen_nodes.append(node)
            kids = [k for k in range(4) if children[node, k] != EMPTY]
            assert len(kids) >= 2
            held += len(kids) - 1
            worst = max(worst, held)
            lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
            for k in kids:
                ch = int(children[node, k])
                if ch >= 0:
                    clo, chi = walk(ch, held)
                else:
                    code = ~ch
                    first, count = code >> 3, (code & 7) + 1
                    clo, chi = np.full(3, np.inf), np.full(3, -np.inf)
                    for j in range(first, first + count):
                        positions.append(j)
                        assert 0 <= j < len(prims)
                        pc = int(prims[j, 0])
                        # the op form of this group lies between its OP_GROUP and that op's skip
                        assert group_ops[gi] < pc < ops[group_ops[gi], 2], f"group {gi}: position {j} names an op outside the group"
                        node_j = int(op_nodes[pc])
                        assert ops[pc, 0] == (OP_SPHERE if nodes[node_j].type == api.RT_NODE_SPHERE else OP_PLANE)
                        assert nodes[node_j].type in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE)
                        plo, phi = _prim_box(desc, node_j)
                        clo, chi = np.minimum(clo, plo), np.maximum(chi, phi)
                        first_guard, n_guard = int(prims[j, 1]), int(prims[j, 2])
                        assert 0 <= first_guard and n_guard >= 0 and first_guard + n_guard <= len(g["guards"])
                        run = g["guards"][first_guard:first_guard + n_guard]
                        assert ((0 <= run) & (run < g["n_bounds"])).all()
                        # a guard is a box test in front of the primitive in the op form too: the same boxes in the same order
                        before = ops[pc - n_guard:pc]
                        assert (before[:, 0] == OP_BOUNDS).all() and (before[:, 1] == run).all()
                b = boxes[node, k].astype(np.float64)
                assert (b[0] <= clo - pad).all() and (b[1] >= chi + pad).all(), f"group {gi} node {node} child {k}: box tighter than the pad"
                lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
            for k in range(4):
                if children[node, k] == EMPTY:
                    assert (boxes[node, k, 0] > boxes[node, k, 1]).all()
            return lo, hi

        lo, hi = walk(n_lo, 0)
        assert sorted(seen_nodes) == list(range(n_lo, n_hi)), f"group {gi}: not every node of its range is reached exactly once"
        assert sorted(positions) == list(range(prim_base, prim_base + len(positions))), f"group {gi}: leaves do not cover its own positions once each"
        prim_base += len(positions)
        # the group's box is the union of its primitives' geometric boxes (rounded outward in f32)
        gb = g64["group_boxes"][gi]
        assert (gb[0] == lo).all() and (gb[1] == hi).all()
        assert (g["group_boxes"][gi][0] <= lo).all() and (g["group_boxes"][gi][1] >= hi).all()
    assert prim_base == len(prims)
    # the stack: what group_search can hold over every root-to-node path, and the level the builder adds to it
    assert worst <= info["group_stack"]
    assert worst + 1 == g["stack_levels"]
    # every group holds each of its primitives once; together they hold every sphere and quad but the lamp and `lost`
    in_groups = {int(op_nodes[pc]) for pc in prims[:, 0]}
    c = gc.case(name)
    leaves = {e.node for e in c.inst}
    lamp = max(leaves)
    dropped = {e.node for e in c.inst if e.kind == api.RT_NODE_SPHERE and e.p[3] == -0.25}
    assert len(dropped) == (1 if name.startswith("two_groups") else 0)
    assert in_groups == leaves - {lamp} - dropped
    assert len(prims) == sum(1 for e in c.inst if e.node in in_groups)


def test_guards_and_second_group_offsets():
    """What the scenes are for is there: a second group with non-zero bases of all four kinds, guard runs in it, and in
    `instanced` two groups over the same description nodes."""
    desc = gc.host_scene("two_groups").desc
    ops, _ = gc.program("two_groups")
    g = api.scene_groups(desc)
    assert g["roots"][1] > 0
    second = g["prims"][40:]                                              # A, 40 spheres, comes first in `world`
    assert (second[:, 1] > 0).all() and (second[:, 2] > 0).any()         # guard_first is rebased; some runs are not empty
    assert len(np.unique(g["prims"][:, 2])) > 1                           # the inverted box gives some primitives more guards
    ranks = ops[g["prims"][:, 0], 2]
    assert len(np.unique(ranks)) == len(ranks) and ranks.min() >= 1       # tie ranks: distinct across both groups
    desc = gc.host_scene("instanced").desc
    op_nodes = api.scene_op_nodes(desc)
    g = api.scene_groups(desc)
    a, b = (sorted(op_nodes[g["prims"][30 * k:30 * (k + 1), 0]]) for k in (0, 1))
    assert a == b and len(set(a)) == 30
    assert len(set(g["prims"][:60, 0])) == 60                             # ... through two op forms


@pytest.mark.parametrize("name", gc.NAMES)
def test_ray_sets(name):
    c = gc.case(name)
    t, gz = c.of("t"), c.of("g")
    # every primitive of every group is the oracle's answer to a target ray; coincident primitives count as one (the one the
    # reference visits later can never be the answer)
    covered = np.zeros(len(c.inst), dtype=bool)
    covered[np.unique(c.target[t & c.on_target])] = True
    key = {}
    for k, e in enumerate(c.inst):
        key.setdefault((e.kind, tuple(np.round(e.to_world(e.p[:3])[0], 9)), abs(float(e.p[3]))), []).append(k)
    for ks in key.values():
        covered[ks] = covered[ks].any()
    op_nodes = api.scene_op_nodes(c.desc)
    in_groups = {int(op_nodes[pc]) for pc in api.scene_groups(c.desc)["prims"][:, 0]}
    required = np.array([e.node in in_groups for e in c.inst])
    share = covered[required].mean()
    print(f"{name}: {len(c.o)} rays, {int(t.sum())} target rays {c.on_target[t].mean():.2%} on target, "
          f"{int(covered[required].sum())} of {int(required.sum())} primitives covered, "
          f"grazing {c.on_target[gz].mean() if gz.any() else float('nan'):.2%} on target, segments {c.seg_occluded.mean():.2%} occluded")
    assert share >= 0.99
    assert gz.any() == (c.n_prims < 200)
    if gz.any():
        assert c.on_target[gz].mean() >= 0.10 and (~c.on_target[gz]).mean() >= 0.10
    assert 0.10 <= c.seg_occluded.mean() <= 0.90
    assert (c.want["klass"] == SURFACE).mean() >= 0.3


def test_duplicate_goes_to_the_group_visited_first():
    """Rays at the two coincident spheres: the oracle answers with dupa's material where A comes first in `world` and with
    dupb's where B does."""
    mats = []
    for name in ("two_groups", "two_groups_swapped"):
        c = gc.case(name)
        dup = [k for k, e in enumerate(c.inst) if e.kind == api.RT_NODE_SPHERE and tuple(e.p[:4]) == (0.0, 1.5, 0.0, 0.5)]
        assert len(dup) == 2 and c.inst[dup[0]].material != c.inst[dup[1]].material
        sel = np.isin(c.target, dup) & c.on_target & c.of("t")
        assert sel.sum() >= gc.K_TARGET
        m = np.unique(c.want["material"][sel])
        assert len(m) == 1
        mats.append(int(m[0]))
    assert mats[0] != mats[1]


@pytest.mark.parametrize("name", [n for n in gc.NAMES if not n.startswith(("lattice", "nodes"))])
def test_f32_sets_are_under_the_cap(name):
    """The f32 rule's own upper bound on what it can excuse (a copy of the ray answers differently), on the oracle alone, for the
    scenes with grazing rays, scale contrast or offsets: under the cap, so the GPU test is not lost before it starts."""
    import f32_ray_bounds as fb
    rs = gc.f32_set(name)
    rs.assert_not_vacuous()
    closest, segments = gc.fragile_shares(name)
    print(f"{name}: fragile share of the closest-hit sample {closest:.2%}, of the segments {segments:.2%}")
    assert closest <= fb.CAP and segments <= fb.CAP
