"""CPU: the leaf-pair / self-collision API surface (pv.LeafPairDistance, ComposedSDF.leaf_pair_distance / leaf_pair_transforms,
RobotSDF.self_collision_*), the default pair rule (model_to_sdf.self_collision_pairs) on chains written here, the argument
checks, and the _lib mirrors of the new C-ABI symbols (include/pvamd.h "Leaf-pair distance").  No GPU: every check here raises or
returns before a kernel is launched."""
import tempfile

import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import model_to_sdf
from pytorch_volumetric_amd import sdf as sdf_mod


def test_exports():
    assert pv.LeafPairDistance is sdf_mod.LeafPairDistance
    assert pv.LeafPairDistance._fields == ("values", "indices", "gradients")
    for name in ("leaf_pair_distance", "leaf_pair_transforms"):
        assert callable(getattr(pv.ComposedSDF, name))
    for name in ("set_self_collision_points", "self_collision_pairs", "self_collision_distance", "link_pair_transforms"):
        assert callable(getattr(pv.RobotSDF, name))
    assert callable(model_to_sdf.self_collision_pairs)


def pairs_of(urdf, names=None):
    chain = pv.build_chain_from_urdf(urdf)
    if names is None:  # one leaf per mesh visual, in frame order (RobotSDF._collect_mesh_links)
        names = [chain.find_frame(n).link.name for n in chain.get_frame_names(exclude_fixed=False)
                 for v in chain.find_frame(n).link.visuals if v.geom_type == "mesh"]
    return model_to_sdf.self_collision_pairs(chain, names), names


def link(name, meshes=1):
    vis = "".join(f'<visual><geometry><mesh filename="{name}_{i}.obj"/></geometry></visual>' for i in range(meshes))
    return f'<link name="{name}">{vis}</link>'


def joint(name, parent, child, kind="revolute"):
    return (f'<joint name="{name}" type="{kind}"><parent link="{parent}"/><child link="{child}"/>'
            f'<origin xyz="0 0 0.1"/><axis xyz="0 0 1"/></joint>')


def unordered(p):
    return {tuple(sorted(x)) for x in p.tolist()}


def test_synthetic_arm_pairs():
    with tempfile.TemporaryDirectory() as tmp:
        chain = W.synthetic_arm(tmp)
    names = [f"link_{i}" for i in range(8)]
    p = model_to_sdf.self_collision_pairs(chain, names)
    assert p.dtype == torch.int64 and p.shape == (42, 2)
    expect = [[s, t] for s in range(8) for t in range(8) if abs(s - t) >= 2]
    assert p.tolist() == expect  # every ordered non-adjacent pair, sorted by (s, t)
    assert len(unordered(p)) == 21


def test_branched_hand():
    urdf = ('<robot name="hand">' + link("base") + link("palm") + link("finger_a") + link("finger_b") + link("tip_a") +
            joint("j0", "base", "palm") + joint("ja", "palm", "finger_a") + joint("jb", "palm", "finger_b") +
            joint("jt", "finger_a", "tip_a") + "</robot>")
    p, names = pairs_of(urdf)
    idx = {n: i for i, n in enumerate(names)}
    got = unordered(p)
    adjacent = {("base", "palm"), ("palm", "finger_a"), ("palm", "finger_b"), ("finger_a", "tip_a")}
    expect = {tuple(sorted((idx[a], idx[b]))) for a in idx for b in idx if a < b and (a, b) not in adjacent and (b, a) not in adjacent}
    assert got == expect
    assert tuple(sorted((idx["finger_a"], idx["finger_b"]))) in got  # the two fingers on one palm are not adjacent
    assert p.tolist() == sorted(p.tolist()) and len(p) == 2 * len(got)


def test_meshless_link_is_collapsed():
    urdf = ('<robot name="r">' + link("l0") + '<link name="bare"/>' + link("l2") + link("l3") +
            joint("j0", "l0", "bare") + joint("j1", "bare", "l2") + joint("j2", "l2", "l3") + "</robot>")
    p, names = pairs_of(urdf)
    assert names == ["l0", "l2", "l3"]
    # l0 is l2's nearest leaf-carrying ancestor: adjacent through the mesh-less link; l0 / l3 are not
    assert p.tolist() == [[0, 2], [2, 0]]


def test_link_with_two_visuals():
    urdf = '<robot name="r">' + link("a", meshes=2) + link("b") + link("c") + joint("j0", "a", "b") + joint("j1", "b", "c") + "</robot>"
    p, names = pairs_of(urdf)
    assert names == ["a", "a", "b", "c"]
    # the two leaves of link a are adjacent to each other and to b; both face c
    assert p.tolist() == [[0, 3], [1, 3], [3, 0], [3, 1]]


def test_unreadable_chain_asks_for_pairs():
    class Opaque:
        pass
    with pytest.raises(ValueError, match="pairs"):
        model_to_sdf.self_collision_pairs(Opaque(), ["a", "b"])


def test_foreign_frame_tree():
    """A pytorch_kinematics-like chain: a root frame with children, each with a link name."""
    class F:
        def __init__(self, name, children=()):
            self.link = type("L", (), {"name": name})()
            self.children = list(children)

    class PK:
        _root = F("base", [F("l1", [F("l2", [F("l3")])])])
    p = model_to_sdf.self_collision_pairs(PK(), ["base", "l1", "l2", "l3"])
    assert unordered(p) == {(0, 2), (0, 3), (1, 3)}


# ---------------------------------------------------------------- argument checks (raise before anything touches a device)
@pytest.fixture()
def composed():
    spheres = [pv.SphereSDF(0.1), pv.SphereSDF(0.2), pv.SphereSDF(0.3)]
    m = torch.eye(4).repeat(3 * 2, 1, 1)
    m[:, 0, 3] = torch.arange(6.0) * 0.1
    c = pv.ComposedSDF(spheres, None)
    c.set_transforms(m, batch_dim=(2,))
    return c


def pts3():
    return [torch.zeros(4, 3), torch.zeros(5, 3), torch.zeros(6, 3)]


def test_same_leaf_pair_raises(composed):
    with pytest.raises(ValueError):
        composed.leaf_pair_distance(pts3(), torch.tensor([[0, 1], [2, 2]]))
    with pytest.raises(ValueError):
        composed.leaf_pair_transforms(torch.tensor([[1, 1]]))


def test_index_out_of_range_raises(composed):
    for bad in ([[0, 3]], [[-1, 0]], [[5, 1]]):
        with pytest.raises(ValueError):
            composed.leaf_pair_distance(pts3(), torch.tensor(bad))
        with pytest.raises(ValueError):
            composed.leaf_pair_transforms(torch.tensor(bad))


def test_pairs_shape_and_dtype(composed):
    for bad in (torch.tensor([0, 1]), torch.tensor([[0, 1, 2]]), torch.tensor([[0.0, 1.0]]), torch.tensor([[True, False]])):
        with pytest.raises(ValueError):
            composed.leaf_pair_distance(pts3(), bad)


def test_last_dimension_raises(composed):
    for bad in (torch.zeros(4, 2), torch.zeros(4, 4), torch.tensor(1.0)):
        pts = pts3()
        pts[1] = bad
        with pytest.raises(ValueError):
            composed.leaf_pair_distance(pts, torch.tensor([[0, 1]]))


def test_leaf_count_must_match(composed):
    with pytest.raises(ValueError):
        composed.leaf_pair_distance(pts3()[:2], torch.tensor([[0, 1]]))
    with pytest.raises(ValueError):
        composed.leaf_pair_distance(torch.zeros(3, 4, 3), torch.tensor([[0, 1]]))


def test_empty_point_set_used_by_a_pair_raises(composed):
    pts = pts3()
    pts[2] = torch.zeros(0, 3)
    with pytest.raises(ValueError, match="empty"):
        composed.leaf_pair_distance(pts, torch.tensor([[0, 1], [1, 2]]))


def test_non_rigid_transforms_raise():
    m = torch.eye(4).repeat(2, 1, 1)
    m[1, 0, 0] = 2.0  # a scale
    c = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], m)
    with pytest.raises(ValueError, match="rigid"):
        c.leaf_pair_distance([torch.zeros(3, 3), torch.zeros(3, 3)], torch.tensor([[0, 1]]))
    with pytest.raises(ValueError, match="rigid"):
        c.leaf_pair_transforms(torch.tensor([[0, 1]]))


def test_no_pairs_give_empty_outputs(composed):
    pts = pts3()
    pts[0] = torch.zeros(0, 3)  # no pair uses it: allowed
    res = composed.leaf_pair_distance(pts, torch.zeros(0, 2, dtype=torch.int64))
    assert isinstance(res, pv.LeafPairDistance)
    assert res.values.shape == (2, 0) and res.indices.shape == (2, 0) and res.gradients.shape == (2, 0, 3)
    assert res.indices.dtype == torch.int64 and res.values.dtype == torch.float32
    res = composed.leaf_pair_distance([p.double() for p in pts], torch.zeros(0, 2, dtype=torch.int64))
    assert res.values.dtype == torch.float64
    assert composed.leaf_pair_transforms(torch.zeros(0, 2, dtype=torch.int64)).shape == (2, 0, 4, 4)


def test_abi_mirrors():
    lib = _lib.load()
    for name in ("pvamd_leaf_pair_scratch_bytes", "pvamd_leaf_pair_transforms", "pvamd_leaf_pair_transforms_f64",
                 "pvamd_leaf_pair_distance", "pvamd_leaf_pair_distance_f64", "pvamd_leaf_pair_distance_backward",
                 "pvamd_leaf_pair_distance_backward_f64"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 16
    # the common case: every set within one 4096-point chunk -> the single-pass forward needs no scratch
    assert _lib.leaf_pair_scratch_bytes(42, 200, 256, False, False) == 0
    assert _lib.leaf_pair_scratch_bytes(42, 200, 4097, False, False) == 16 * 42 * 200 * 2
    assert _lib.leaf_pair_scratch_bytes(42, 200, 256, True, True) == 24 * 42 * 200 * 8
    # these values come from the library: tests/test_abi.py compares the header's macro with the exported function
    assert _lib.leaf_pair_scratch_bytes(3, 7, 4096, True, False) == 0
    assert _lib.leaf_pair_scratch_bytes(1, 65535, 1 << 20, False, False) == 16 * 65535 * 256
    assert lib.pvamd_leaf_pair_scratch_bytes(0, 200, 256, 0, 0) == 0
    assert lib.pvamd_leaf_pair_scratch_bytes(42, 0, 256, 0, 1) == 0


def test_c_entry_points_check_arguments_before_launching():
    """Shape and mode errors come back as codes without touching a device pointer."""
    lib = _lib.load()
    null = None
    for f in (lib.pvamd_leaf_pair_transforms, lib.pvamd_leaf_pair_transforms_f64):
        assert f(null, 0, 4, null, 3, null, null) == _lib.E_SHAPE  # S = 0
        assert f(null, 8, 0, null, 3, null, null) == _lib.E_SHAPE  # A = 0
        assert f(null, 8, 4, null, 0, null, null) == 0             # K = 0: nothing to do
        assert f(null, 8, 4, null, 3, null, null) == -1  # PVAMD_E_NULL
    for f in (lib.pvamd_leaf_pair_distance, lib.pvamd_leaf_pair_distance_f64):
        assert f(null, 8, null, 4, null, 0, null, 3, 1, 0, null, null, null, null, null) == _lib.E_SHAPE  # no points
        assert f(null, 8, null, 4, null, 10, null, 3, 11, 0, null, null, null, null, null) == _lib.E_SHAPE  # max_points > npoints
        assert f(null, 8, null, 4, null, 10, null, 3, 5, 2, null, null, null, null, null) == -4  # PVAMD_E_MODE  # no such leaf mode
        assert f(null, 8, null, 4, null, 10, null, 3, 5, 0, null, null, null, null, null) == -1  # PVAMD_E_NULL
    for f in (lib.pvamd_leaf_pair_distance_backward, lib.pvamd_leaf_pair_distance_backward_f64):
        assert f(null, 65, null, null, 4, null, 10, null, 3, 0, null, null, null, null, null, null) == _lib.E_SHAPE  # S > 64
        assert f(null, 8, null, null, 4, null, 10, null, 3, 0, null, null, null, null, null, null) == -1  # PVAMD_E_NULL
