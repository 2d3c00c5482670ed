"""CPU: forward kinematics of a branching tree with prismatic and fixed joints, links with several mesh visuals and mesh-less
frames -- Chain.joint_table, Chain.forward_kinematics and the CPU oracle of csrc/fk.hip against tests/fk_ref.py, a float64
walk of a literal table that goes through neither kinematics.Chain nor transforms.  (The kernels: tests/test_fk_gpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import oracle
from pytorch_volumetric_amd import kinematics
from tests import fk_ref as R

FK_TOL = 2e-6  # the project's bound for float32 FK against a float64 one (test_robot_gpu.py, test_host_logic.py)


def tree_chain(dtype=torch.float32):
    leaves = R.leaf_links(R.TREE)
    return kinematics.build_chain_from_urdf(R.urdf(R.TREE, [f"m{s}.obj" for s in range(len(leaves))]), dtype=dtype)


def static_chain(dtype=torch.float32):
    return kinematics.build_chain_from_urdf(R.urdf(R.STATIC, ["m0.obj", "m1.obj"]), dtype=dtype)


def records(raw):
    F = len(raw) // ctypes.sizeof(pv._lib.JointDesc)
    arr = (pv._lib.JointDesc * F).from_buffer_copy(raw)
    return [(r.parent, r.jtype, r.jcol, r.leaf_slot) for r in arr], arr


# a leaf order that is not the frame order: the duplicates of `shoulder` and `palm` get slots far apart and out of order
PERMUTED = [5, 9, 2, 11, 0, 7, 3, 6, 10, 1, 8, 4]


def permuted_leaves():
    frame_order = R.leaf_links(R.TREE)
    return [frame_order[i] for i in PERMUTED]


def test_reference_tables_are_the_robots_the_tests_are_about():
    """What the other tests count on, stated from the literal tables: 12 frames, 8 joints, 12 leaves; the frame order is not the
    declaration order (antenna, a child of shoulder, comes before head, a child of torso)."""
    assert R.frame_names(R.TREE) == ["base", "torso", "lift", "shoulder", "elbow", "palm", "finger_a", "tip_a", "finger_b",
                                     "antenna", "head", "camera"]
    assert R.joint_names(R.TREE) == ["j_lift", "j_shoulder", "j_elbow", "j_palm", "j_finger_a", "j_finger_b", "j_antenna",
                                     "j_head"]
    assert R.prismatic_columns(R.TREE) == [0, 4, 5]
    assert len(R.leaf_links(R.TREE)) == 12 and sorted(PERMUTED) == list(range(12))
    assert len(R.frame_names(R.STATIC)) == 3 and R.joint_names(R.STATIC) == [] and len(R.leaf_links(R.STATIC)) == 2
    # Rz Ry Rx of the origin, on one hand-computed case: roll = pi/2 takes y to z, then yaw = pi/2 takes x to y
    m = R.origin64((1, 2, 3), (np.pi / 2, 0, np.pi / 2))
    assert np.allclose(m[:3, :3] @ [0, 1, 0], [0, 0, 1], atol=1e-15) and np.allclose(m[:3, :3] @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    assert np.array_equal(m[:3, 3], [1, 2, 3])
    # Rodrigues about z by +90 degrees takes x to y; a prismatic joint moves along the NORMALISED axis
    q = np.zeros((1, 8))
    q[0, 7] = np.pi / 2  # head: continuous about z
    q[0, 4] = 0.2        # finger_a: prismatic along (0, 1, 0.5) / |.|
    w0, w1 = R.fk64(R.TREE, np.zeros((1, 8))), R.fk64(R.TREE, q)
    names = R.frame_names(R.TREE)
    head, fa = names.index("head"), names.index("finger_a")
    assert np.allclose(w0[head, 0, :3, :3].T @ w1[head, 0, :3, :3] @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    step = w0[fa, 0, :3, :3].T @ (w1[fa, 0, :3, 3] - w0[fa, 0, :3, 3])
    assert np.allclose(step, 0.2 * np.array([0, 1, 0.5]) / np.sqrt(1.25), atol=1e-15)


@pytest.mark.parametrize("order", ["frame", "permuted"])
def test_joint_table_structure_of_the_tree(order):
    """parent, jtype, jcol and leaf_slot of every record of Chain.joint_table, the record count and the joint name order, from
    fk_ref's table: 12 frames + 2 duplicates of shoulder + 1 of palm = 15 records."""
    chain = tree_chain()
    leaves = R.leaf_links(R.TREE) if order == "frame" else permuted_leaves()
    got, arr = records(chain.joint_table(leaves))
    want = R.expected_records(R.TREE, leaves)
    assert len(want) == 15 and len(got) == len(want)
    assert got == want
    assert chain.get_joint_parameter_names() == R.joint_names(R.TREE) and chain.n_joints == 8
    assert chain.get_frame_names(exclude_fixed=False) == R.frame_names(R.TREE)
    # the cases the kernels' parent rule is about, spelled out (record numbers are those of the 15-record table)
    parents = [r[0] for r in got]
    assert parents[4] == 3 and parents[5] == 3        # the duplicates of shoulder; record 5's parent is f - 2
    assert parents[6] == 3 and parents[12] == 3       # elbow and antenna: two children of a branching link
    assert parents[8] == 7 and parents[11] == 7       # the duplicate of palm; finger_b, palm's second child
    assert parents[13] == 1 and parents[0] == -1      # head hangs off torso, twelve records back
    assert [r[2] for r in got if r[1]] == list(range(8))
    assert sorted(r[3] for r in got if r[3] >= 0) == list(range(12)) and [r[3] for r in got].count(-1) == 3
    if order == "permuted":
        slots = [r[3] for r in got if r[3] >= 0]
        assert slots != sorted(slots)  # the slots are not in record order
    # axes are normalised, origins are the table's, duplicates are identity
    own, dups = R.frame_records(R.TREE, leaves)
    assert len(own) == 12 and dups == {4: "shoulder", 5: "shoulder", 8: "palm"}
    for row, i in zip(R.frames(R.TREE), own):
        o = np.array(list(arr[i].origin)).reshape(3, 4)
        assert np.abs(o - R.origin64(row[4], row[5])[:3]).max() < 1e-7
        if row[2] in (R.REVOLUTE, R.CONTINUOUS, R.PRISMATIC):
            k = np.asarray(row[3], dtype=np.float64)
            assert np.abs(np.array(list(arr[i].axis)) - k / np.linalg.norm(k)).max() < 1e-7
    for i in dups:
        assert list(arr[i].origin) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("scale", [0.8, 3.0, 50.0])
def test_chain_fk_in_float64_equals_the_reference(scale):
    chain = tree_chain(torch.float64)
    q = R.draw_q(R.TREE, 50, scale, seed=11)
    fk = chain.forward_kinematics(torch.tensor(q, dtype=torch.float64))
    ref = R.fk64(R.TREE, q)
    worst = max(np.abs(fk[name].get_matrix().numpy() - ref[f]).max() for f, name in enumerate(R.frame_names(R.TREE)))
    print(f"Chain.forward_kinematics float64 vs fk64, scale {scale}: {worst:.2e}")
    assert worst < 1e-12


@pytest.mark.parametrize("order", ["frame", "permuted"])
@pytest.mark.parametrize("scale", [0.8, 3.0, 50.0])
def test_oracle_fk_and_stack_equal_the_reference(scale, order):
    """oracle_chain_fk and oracle.transform_stack on joint_table's bytes against fk64 / stack64 of the float32 joint values, at
    A = 200.  No frame can be further from the base than 1.55 (the origin lengths plus 0.3 per prismatic joint along the longest
    branch), so 2e-6 is some twenty float32 roundings of the largest entry."""
    chain = tree_chain()
    A = 200
    leaves = R.leaf_links(R.TREE) if order == "frame" else permuted_leaves()
    q = R.draw_q(R.TREE, A, scale, seed=int(scale * 10)).astype(np.float32)
    world, link_world, _, _ = oracle.chain_fk(chain.joint_table(leaves), q, len(leaves))
    ref = R.fk64(R.TREE, q)
    assert world.shape == (12 + 3, A, 3, 4)
    own, dups = R.frame_records(R.TREE, leaves)
    err_frames = max(np.abs(world[i] - ref[f, :, :3, :]).max() for f, i in enumerate(own))
    # a duplicate record is its link's frame again
    names = R.frame_names(R.TREE)
    for i, link in dups.items():
        assert np.array_equal(world[i], world[own[names.index(link)]])
    err_leaves = np.abs(link_world - R.leaf_world64(R.TREE, q, leaves)).max()
    offsets = R.visual_offsets64(R.TREE)
    if order == "permuted":
        offsets = offsets[PERMUTED]
    off_inv = np.linalg.inv(offsets).astype(np.float32)
    stack = oracle.transform_stack(off_inv, link_world, len(leaves), A)
    err_stack = np.abs(stack - R.stack64(R.TREE, q, offsets, leaves)).max()
    print(f"oracle vs float64, scale {scale}, {order} order: frames {err_frames:.2e} leaves {err_leaves:.2e} stack {err_stack:.2e}; "
          f"max |t| {np.abs(ref[:, :, :3, 3]).max():.3f}")
    assert np.abs(ref[:, :, :3, 3]).max() < 1.55
    assert err_frames < FK_TOL and err_leaves < FK_TOL and err_stack < FK_TOL


@pytest.mark.parametrize("A", [1, 3])
def test_static_robot_through_the_oracle_with_no_joint_values(A):
    """M == 0: a robot of fixed joints only.  oracle.chain_fk takes A from q's leading dimension (it used to infer A = 0 from
    q's size), and every configuration is the same frames."""
    chain = static_chain()
    assert chain.get_joint_parameter_names() == [] and chain.n_joints == 0
    leaves = R.leaf_links(R.STATIC)
    assert leaves == ["pedestal", "plate"]
    raw = chain.joint_table(leaves)
    got, _ = records(raw)
    assert got == R.expected_records(R.STATIC) == [(-1, 0, -1, 0), (0, 0, -1, -1), (1, 0, -1, 1)]
    q = np.zeros((A, 0), np.float32)
    world, link_world, sq, cq = oracle.chain_fk(raw, q, len(leaves))
    assert world.shape == (3, A, 3, 4) and link_world.shape == (2 * A, 4, 4) and sq.shape == (A, 0) and cq.shape == (A, 0)
    ref = R.fk64(R.STATIC, q)
    assert ref.shape == (3, A, 4, 4)
    assert np.abs(world - ref[:, :, :3, :]).max() < FK_TOL
    assert np.abs(link_world - R.leaf_world64(R.STATIC, q)).max() < FK_TOL
    assert all(np.array_equal(world[:, a], world[:, 0]) for a in range(A))
    offsets = R.visual_offsets64(R.STATIC)
    stack = oracle.transform_stack(np.linalg.inv(offsets).astype(np.float32), link_world, 2, A)
    assert np.abs(stack - R.stack64(R.STATIC, q, offsets)).max() < FK_TOL
    # the frames are not trivial: both fixed origins moved the plate
    assert np.abs(ref[2, 0, :3, 3]).min() > 0.01 and np.abs(ref[2, 0, :3, :3] - np.eye(3)).max() > 0.1
    if A == 1:  # a flat (0,) vector is one configuration
        w1, _, _, _ = oracle.chain_fk(raw, np.zeros((0,), np.float32), len(leaves))
        assert np.array_equal(w1, world)


def test_oracle_chain_fk_takes_the_batch_from_the_leading_dimensions():
    chain = tree_chain()
    leaves = R.leaf_links(R.TREE)
    q = R.draw_q(R.TREE, 6, 0.8, seed=2).astype(np.float32)
    w, lw, _, _ = oracle.chain_fk(chain.joint_table(leaves), q, 12)
    w2, lw2, _, _ = oracle.chain_fk(chain.joint_table(leaves), q.reshape(2, 3, 8), 12)
    assert w.shape == (15, 6, 3, 4) and np.array_equal(w, w2) and np.array_equal(lw, lw2)
    w1, _, _, _ = oracle.chain_fk(chain.joint_table(leaves), q[0], 12)
    assert np.array_equal(w1[:, 0], w[:, 0])


# ---- the tree robot with meshes: what tests/test_fk_gpu.py queries, and the part of it that needs no GPU ----
RES, PADDING = 0.02, 0.1          # cache_link_sdf_factory(resolution=RES, padding=PADDING)
BOUNDARY_TOL = 2e-6               # a probe point this close to a voxel boundary of its own leaf may be excluded
PROBE_POINTS, PROBE_SEED, PROBE_Q_SEED = 300, 7, 21


def leaf_radii(s):
    """A different ellipsoid for every leaf, so that a swapped slot changes answers."""
    return 0.03 + 0.004 * s, 0.055 - 0.002 * s, 0.035 + 0.003 * ((5 * s) % 12)


def write_robot(table, directory):
    """One ellipsoid mesh file per leaf in `directory`; returns the URDF text."""
    from pytorch_volumetric_amd import mesh_io
    names = []
    for s in range(len(R.leaf_links(table))):
        mesh = mesh_io.uv_sphere_mesh(1.0, 12, 6, scale=leaf_radii(s), center=(0.0, 0.005 * (s % 3), 0.01 * (s % 4)))
        names.append(f"leaf_{s}.obj")
        mesh_io.save_obj(f"{directory}/{names[-1]}", mesh)
    return R.urdf(table, names)


def leaf_cache_view(directory, s):
    """The surface bounding box and the value-range view of leaf s's cache, as CachedSDF derives them from the mesh file."""
    from pytorch_volumetric_amd.voxel import RangeView
    obj = pv.MeshObjectFactory(f"leaf_{s}.obj", path_prefix=str(directory))
    ranges = pv.get_divisible_range_by_resolution(RES, obj.bounding_box(padding=PADDING))
    coords, _ = pv.get_coordinates_and_points_in_grid(RES, ranges, get_points=False)
    return obj.bounding_box(padding=0.0), RangeView(ranges, [len(c) for c in coords])


def probe_points(table, directory, q_row):
    """Per leaf: PROBE_POINTS points inside its own surface bounding box, in its own frame (float64); their images in the world
    under joint values q_row, by fk64 @ offset in float64; their voxel in the leaf's own cache (float64 index arithmetic);
    and which of them lie within BOUNDARY_TOL of a voxel boundary (a half-cell plane of the nearest lookup) along some axis."""
    names, offsets = R.frame_names(table), R.visual_offsets64(table)
    world = R.fk64(table, q_row)
    rng = np.random.default_rng(PROBE_SEED)
    out = []
    for s, link in enumerate(R.leaf_links(table)):
        bb, view = leaf_cache_view(directory, s)
        assert view.index_f64
        local = rng.uniform(bb[:, 0], bb[:, 1], (PROBE_POINTS, 3))
        m = world[names.index(link), 0] @ offsets[s]
        cell = (local - view.dmin.numpy()) / view.dres.numpy()
        voxel = np.rint(cell).astype(np.int64)
        assert (voxel >= 0).all() and (voxel < np.array(view.shape)).all()
        to_boundary = np.abs(cell - np.floor(cell) - 0.5) * view.dres.numpy()
        out.append(dict(local=local, world=local @ m[:3, :3].T + m[:3, 3], voxel=voxel, view=view,
                        excluded=(to_boundary < BOUNDARY_TOL).any(axis=1)))
    return out


def probe_q():
    return R.draw_q(R.TREE, 1, 0.8, PROBE_Q_SEED).astype(np.float32)


def test_probe_points_of_the_gpu_test_stay_clear_of_voxel_boundaries(tmp_path):
    """The one-sided bound of test_fk_gpu (robot value <= the leaf's own value at points placed by the float64 reference) may
    leave out points within 2e-6 of a voxel boundary, 2 % at the most.  Which points those are follows from the float64
    reference and the cache geometry alone: with this seed it is far fewer (expected 3 axes x 4e-6 / 0.02 = 0.06 %)."""
    write_robot(R.TREE, tmp_path)
    probes = probe_points(R.TREE, tmp_path, probe_q())
    assert len(probes) == 12
    excluded = np.concatenate([p["excluded"] for p in probes])
    assert excluded.shape == (12 * PROBE_POINTS,) and excluded.mean() <= 0.02
    assert all(p["excluded"].mean() <= 0.02 for p in probes)
    # the probe is about twelve different leaves placed apart
    centres = np.stack([p["world"].mean(axis=0) for p in probes])
    assert len({leaf_radii(s) for s in range(12)}) == 12
    assert min(np.linalg.norm(centres[i] - centres[j]) for i in range(12) for j in range(i)) > 5e-3
