"""CPU: the leaf-pair hinge API surface (pv.LeafPairHinge, ComposedSDF.leaf_pair_hinge, RobotSDF.self_collision_hinge), the
argument checks, and the _lib mirrors of the new C-ABI symbols (include/pvamd.h "Leaf-pair hinge").  No GPU: every check here
raises or returns before a kernel is launched."""
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import sdf as sdf_mod

NAMES = ("pvamd_leaf_pair_hinge_scratch_bytes", "pvamd_leaf_pair_hinge", "pvamd_leaf_pair_hinge_f64",
         "pvamd_leaf_pair_hinge_backward", "pvamd_leaf_pair_hinge_backward_f64")


def test_exports():
    assert pv.LeafPairHinge is sdf_mod.LeafPairHinge
    assert pv.LeafPairHinge._fields == ("values", "counts")
    assert callable(pv.ComposedSDF.leaf_pair_hinge)
    assert callable(pv.RobotSDF.self_collision_hinge)


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


PAIRS = torch.tensor([[0, 1], [2, 0]])


@pytest.mark.parametrize("margin", ["0.1", None, torch.tensor(0.1), True, 1j])
def test_margin_type_raises(composed, margin):
    with pytest.raises(TypeError):
        composed.leaf_pair_hinge(pts3(), PAIRS, margin)


@pytest.mark.parametrize("margin", [float("inf"), float("-inf"), float("nan")])
def test_margin_must_be_finite(composed, margin):
    with pytest.raises(ValueError, match="finite"):
        composed.leaf_pair_hinge(pts3(), PAIRS, margin)


@pytest.mark.parametrize("power", [0, 3, 1.5, True, "2"])
def test_power_raises(composed, power):
    with pytest.raises(ValueError, match="power"):
        composed.leaf_pair_hinge(pts3(), PAIRS, 0.1, power=power)


def test_same_leaf_and_out_of_range_pairs_raise(composed):
    for bad in ([[0, 1], [2, 2]], [[0, 3]], [[-1, 0]]):
        with pytest.raises(ValueError):
            composed.leaf_pair_hinge(pts3(), torch.tensor(bad), 0.1)


def test_empty_point_set_used_by_a_pair_raises(composed):
    pts = pts3()
    pts[1] = torch.zeros(0, 3)
    with pytest.raises(ValueError, match="empty"):
        composed.leaf_pair_hinge(pts, PAIRS, 0.1)


def test_non_rigid_transforms_raise():
    m = torch.eye(4).repeat(2, 1, 1)
    m[1, 0, 0] = 2.0  # a scale
    c = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], m)
    with pytest.raises(ValueError, match="rigid"):
        c.leaf_pair_hinge([torch.zeros(3, 3), torch.zeros(3, 3)], torch.tensor([[0, 1]]), 0.1)


def test_missing_transforms_raise():
    c = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
    with pytest.raises(ValueError, match="transforms"):
        c.leaf_pair_hinge([torch.zeros(3, 3), torch.zeros(3, 3)], torch.tensor([[0, 1]]), 0.1)


def test_no_pairs_give_empty_outputs(composed):
    pts = pts3()
    pts[0] = torch.zeros(0, 3)  # no pair uses it: allowed
    none = torch.zeros(0, 2, dtype=torch.int64)
    res = composed.leaf_pair_hinge(pts, none, 0.1)
    assert isinstance(res, pv.LeafPairHinge)
    assert res.values.shape == (2, 0) and res.counts.shape == (2, 0)
    assert res.values.dtype == torch.float32 and res.counts.dtype == torch.int64
    res = composed.leaf_pair_hinge([p.double() for p in pts], none, 0.1, power=1)
    assert res.values.shape == (2, 0) and res.values.dtype == torch.float64 and res.counts.dtype == torch.int64


def test_abi_mirrors():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 16
    # every set within one 4096-point chunk: the single-pass forward needs no scratch
    assert _lib.leaf_pair_hinge_scratch_bytes(42, 200, 4096, False, False) == 0
    assert _lib.leaf_pair_hinge_scratch_bytes(42, 200, 4097, False, False) == 16 * 42 * 200 * 2
    assert _lib.leaf_pair_hinge_scratch_bytes(42, 200, 256, False, True) == 42 * 200 * 12 * 4 + 24 * 42 * 200 * 4
    # These values come from the library (tests/test_abi.py: the binding only calls it).  The backward worked by hand at the
    # chunk boundary: the dC slab [K][A][chunks of 1024][12] rounded up to 256 B, then dMs and dMt.
    assert _lib.leaf_pair_hinge_scratch_bytes(2, 3, 1024, False, True) == 512 + 24 * 2 * 3 * 4
    assert _lib.leaf_pair_hinge_scratch_bytes(2, 3, 1025, False, True) == 768 + 24 * 2 * 3 * 4
    assert _lib.leaf_pair_hinge_scratch_bytes(2, 3, 1025, True, True) == 1280 + 24 * 2 * 3 * 8
    assert lib.pvamd_leaf_pair_hinge_scratch_bytes(0, 200, 256, 0, 0) == 0
    assert lib.pvamd_leaf_pair_hinge_scratch_bytes(42, 0, 256, 0, 1) == 0


def test_c_entry_points_check_arguments_before_launching():
    """Shape, mode and NULL errors come back as codes without touching a device pointer."""
    lib = _lib.load()
    null = None
    for f in (lib.pvamd_leaf_pair_hinge, lib.pvamd_leaf_pair_hinge_f64):
        assert f(null, 8, null, 4, null, 0, null, 3, 1, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # no points
        assert f(null, 8, null, 4, null, 10, null, 3, 11, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # max_points > npoints
        assert f(null, 0, null, 4, null, 10, null, 3, 5, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # S = 0
        assert f(null, 8, null, 4, null, 10, null, 70000, 5, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # K > 65535
        assert f(null, 8, null, 4, null, 10, null, 3, 5, 2, 0.1, 2, null, null, null, null) == -4  # PVAMD_E_MODE: leaf mode
        assert f(null, 8, null, 4, null, 10, null, 3, 5, 0, 0.1, 3, null, null, null, null) == -4  # PVAMD_E_MODE: power
        assert f(null, 8, null, 4, null, 10, null, 3, 5, 0, 0.1, 2, null, null, null, null) == -1  # PVAMD_E_NULL
        assert f(null, 8, null, 4, null, 10, null, 0, 5, 0, 0.1, 2, null, null, null, null) == 0   # K = 0: nothing to do
    for f in (lib.pvamd_leaf_pair_hinge_backward, lib.pvamd_leaf_pair_hinge_backward_f64):
        assert f(null, 65, null, null, 4, null, 10, null, 3, 5, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # S > 64
        assert f(null, 8, null, null, 4, null, 10, null, 3, 11, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE
        assert f(null, 8, null, null, 4, null, 10, null, 3, 5, 1, 0.1, 0, null, null, null, null) == -4  # PVAMD_E_MODE: power
        assert f(null, 8, null, null, 4, null, 10, null, 3, 5, 0, 0.1, 2, null, null, null, null) == -1  # PVAMD_E_NULL
