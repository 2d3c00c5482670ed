"""CPU: the hinge_over_points API surface (pv.HingeOverPoints, ComposedSDF / RobotSDF.hinge_over_points), its argument checks,
P = 0 giving zeros, and the _lib mirrors of the new C-ABI symbols and scratch macros (include/pvamd.h "Hinge penalty over
points").  No GPU: every check here raises or returns before a kernel is launched."""
import math

import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import sdf as sdf_mod


def test_exports():
    assert pv.HingeOverPoints is sdf_mod.HingeOverPoints
    assert pv.HingeOverPoints._fields == ("values", "counts")
    assert callable(pv.ComposedSDF.hinge_over_points)
    assert callable(pv.RobotSDF.hinge_over_points)


@pytest.fixture()
def composed():
    spheres = [pv.SphereSDF(0.1), pv.SphereSDF(0.2)]
    m = torch.eye(4).repeat(2 * 3, 1, 1)
    m[:, 0, 3] = torch.arange(6.0) * 0.1
    c = pv.ComposedSDF(spheres, None)
    c.set_transforms(m, batch_dim=(3,))
    return c


def test_power_must_be_one_or_two(composed):
    for bad in (0, 3, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError):
            composed.hinge_over_points(torch.zeros(4, 3), 0.1, power=bad)


def test_margin_must_be_a_finite_real(composed):
    for bad in (math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError):
            composed.hinge_over_points(torch.zeros(4, 3), bad)
    for bad in (torch.tensor(0.1), "0.1", None, [0.1], True, 1j):
        with pytest.raises(TypeError):
            composed.hinge_over_points(torch.zeros(4, 3), bad)


def test_per_leaf_must_be_a_bool(composed):
    for bad in (1, 0, "yes", None, 2.0):
        with pytest.raises(TypeError):
            composed.hinge_over_points(torch.zeros(4, 3), 0.1, per_leaf=bad)


def test_last_dimension_must_be_three(composed):
    for pts in (torch.zeros(5, 2), torch.zeros(5, 4), torch.zeros(2), torch.tensor(1.0)):
        with pytest.raises(ValueError):
            composed.hinge_over_points(pts, 0.1)


def test_transforms_must_be_set():
    c = pv.ComposedSDF([pv.SphereSDF(0.1)], None)
    with pytest.raises(ValueError):
        c.hinge_over_points(torch.zeros(4, 3), 0.1)


@pytest.mark.parametrize("per_leaf", [False, True])
def test_no_points_give_zeros(composed, per_leaf):
    for pts in (torch.empty(0, 3), torch.empty(2, 0, 3), torch.empty(0, 3, dtype=torch.float64)):
        for power in (1, 2):
            res = composed.hinge_over_points(pts, 0.25, power=power, per_leaf=per_leaf)
            assert isinstance(res, pv.HingeOverPoints)
            shape = (3, 2) if per_leaf else (3,)
            assert res.values.shape == shape and res.counts.shape == shape
            assert res.counts.dtype == torch.int64
            assert not res.values.any() and not res.counts.any()
            assert res.values.dtype == (torch.float64 if pts.dtype == torch.float64 else torch.float32)


def test_abi_mirrors():
    assert _lib.hinge_over_points_scratch_bytes(8, 200, 262144, False) == 16 * 200 * 64
    assert _lib.hinge_over_points_scratch_bytes(8, 200, 262145, True) == 16 * 200 * 8 * 65
    # C4: 256 backward chunks, 8 splits of 25 configurations: slab 256 x 8 x 200 x 12 x 4 B plus 8 split rows of dpoints
    assert _lib.hinge_over_points_backward_scratch_bytes(8, 200, 262144, False, False) == \
        256 * 8 * 200 * 12 * 4 + 8 * 262144 * 3 * 4
    lib = _lib.load()
    for name in ("pvamd_hinge_over_points_scratch_bytes", "pvamd_hinge_over_points_backward_scratch_bytes",
                 "pvamd_composed_hinge_over_points", "pvamd_composed_hinge_over_points_f64",
                 "pvamd_composed_hinge_over_points_backward", "pvamd_composed_hinge_over_points_backward_f64"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # The sizes come from the library (tests/test_abi.py: the binding only calls it; the forward's macro against the function).
    # The backward's plan, worked by hand where its layout changes: slab [chunks of 1024][S A][12] rounded up to 256 B, split
    # rows [nsplit][P][3] when the configurations are split, one more [P][3] behind a 256 B boundary for per_leaf with S > 1.
    bwd = _lib.hinge_over_points_backward_scratch_bytes
    assert bwd(1, 1, 1000, False, False) == 256                                       # one chunk, no split: 48 B of slab
    assert bwd(2, 3, 1025, False, False) == 768 + 3 * 1025 * 3 * 4                    # two chunks, one configuration per split
    assert bwd(2, 64, 33792, False, False) == 33 * 2 * 64 * 12 * 4 + 32 * 33792 * 3 * 4  # 33 chunks: two configurations per split
    assert bwd(2, 3, 1025, True, True) == 74752 + 1025 * 3 * 8                        # one-leaf plan 768 + 73800, rounded up
    assert bwd(1, 3, 1025, True, True) == 768 + 3 * 1025 * 3 * 8                      # one leaf: no leaf term
    # no pairs or no points: nothing to size
    assert lib.pvamd_hinge_over_points_scratch_bytes(8, 200, 0, 0) == 0
    assert lib.pvamd_hinge_over_points_backward_scratch_bytes(8, 0, 10, 0, 0) == 0


def test_c_entry_points_check_arguments_before_launching():
    """Shape, mode and power errors come back as codes without touching a device pointer."""
    lib = _lib.load()
    null = None
    for f in (lib.pvamd_composed_hinge_over_points, lib.pvamd_composed_hinge_over_points_f64):
        assert f(null, 8, null, 4, null, 0, 0, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # P = 0
        assert f(null, 0, null, 4, null, 10, 0, 0, 0.1, 2, null, null, null, null) == _lib.E_SHAPE  # S = 0
        assert f(null, 8, null, 4, null, 10, 0, 0, 0.1, 3, null, null, null, null) != 0  # power 3
        assert f(null, 8, null, 4, null, 10, 2, 0, 0.1, 2, null, null, null, null) != 0  # no such leaf mode
    for f in (lib.pvamd_composed_hinge_over_points_backward, lib.pvamd_composed_hinge_over_points_backward_f64):
        assert f(null, 65, null, 4, null, 10, 0, 0, 0.1, 2, null, null, null, null, null) == _lib.E_SHAPE  # S > 64
        assert f(null, 8, null, 4, null, 10, 0, 0, 0.1, 0, null, null, null, null, null) != 0  # power 0
