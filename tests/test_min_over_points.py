"""CPU: the min_over_points API surface (pv.MinOverPoints, ComposedSDF / RobotSDF.min_over_points), its argument checks, and the
index rule of include/pvamd.h "Minimum over points" -- NaN lowest, -0.0 and +0.0 tie, the smallest index among the minima --
restated on order-preserving keys and checked against hand-made cases, together with the torch statement the generic path
uses (sdf.first_argmin).  No GPU: every check here raises or returns before a kernel is launched."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import sdf as sdf_mod


def key_argmin(v):
    """The rule as the kernels state it: key = order-preserving bits of the value (NaN -> 0, -0 -> +0), then the index."""
    v = np.asarray(v, dtype=np.float64)
    best = None
    for i, x in enumerate(v):
        if math.isnan(x):
            k = 0
        else:
            u = int(np.array(0.0 if x == 0 else x, np.float64).view(np.uint64))
            k = (~u & 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | (1 << 63))
        if best is None or (k, i) < best:
            best = (k, i)
    return best[1]


HAND = [
    ([3.0, 1.0, 2.0], 1),
    ([1.0, 1.0, 0.5, 0.5], 2),                      # ties: the smallest index
    ([0.0, -0.0, 1.0], 0),                          # -0 and +0 tie
    ([-0.0, 0.0], 0),
    ([2.0, 0.0, -0.0, -1e-45], 3),                  # the smallest negative denormal is below both zeros
    ([1.0, math.nan, -5.0, math.nan], 1),           # NaN counts as the minimum, the first NaN wins
    ([math.inf, math.inf], 0),
    ([math.inf, -math.inf, -math.inf], 1),
    ([-1.0], 0),
    ([5.0, 4.0, 3.0, 2.0, 1.0, 1.0], 4),
]


@pytest.mark.parametrize("vals,want", HAND)
def test_index_rule_on_hand_cases(vals, want):
    assert key_argmin(vals) == want
    for dt in (torch.float32, torch.float64):
        assert int(sdf_mod.first_argmin(torch.tensor(vals, dtype=dt))) == want


def test_index_rule_batched_against_restatement():
    g = torch.Generator().manual_seed(0)
    v = torch.randint(-3, 4, (64, 33), generator=g).double() * 0.5
    v[v == 0] = torch.where(torch.rand(int((v == 0).sum()), generator=g) < 0.5, -0.0, 0.0).double()
    v[torch.rand(v.shape, generator=g) < 0.01] = math.nan
    got = sdf_mod.first_argmin(v)
    assert got.dtype == torch.int64 and got.shape == (64,)
    for a in range(v.shape[0]):
        assert int(got[a]) == key_argmin(v[a].numpy())


def test_exports():
    assert pv.MinOverPoints is sdf_mod.MinOverPoints
    assert pv.MinOverPoints._fields == ("values", "indices", "gradients")
    assert callable(pv.ComposedSDF.min_over_points)
    assert callable(pv.RobotSDF.min_over_points)


@pytest.fixture()
def composed():
    spheres = [pv.SphereSDF(0.1), pv.SphereSDF(0.2)]
    m = torch.eye(4).repeat(2 * 3, 1, 1)
    m[:, 0, 3] = torch.arange(6.0) * 0.1
    c = pv.ComposedSDF(spheres, None)
    c.set_transforms(m, batch_dim=(3,))
    return c


def test_zero_points_raise(composed):
    for pts in (torch.empty(0, 3), torch.empty(2, 0, 3)):
        with pytest.raises(ValueError):
            composed.min_over_points(pts)
        with pytest.raises(ValueError):
            composed.min_over_points(pts, per_leaf=True)


def test_last_dimension_must_be_three(composed):
    for pts in (torch.zeros(5, 2), torch.zeros(5, 4), torch.zeros(2), torch.tensor(1.0)):
        with pytest.raises(ValueError):
            composed.min_over_points(pts)


def test_per_leaf_must_be_a_bool(composed):
    for bad in (1, 0, "yes", None, 2.0):
        with pytest.raises(TypeError):
            composed.min_over_points(torch.zeros(4, 3), per_leaf=bad)


def test_transforms_must_be_set():
    c = pv.ComposedSDF([pv.SphereSDF(0.1)], None)
    with pytest.raises(ValueError):
        c.min_over_points(torch.zeros(4, 3))


def test_abi_mirrors():
    from pytorch_volumetric_amd import _lib
    assert _lib.LEAF_MODES == {"nearest": 0, "trilinear": 1}
    assert _lib.min_over_points_scratch_bytes(8, 200, 262144, False) == 16 * 200 * 64
    assert _lib.min_over_points_scratch_bytes(8, 200, 262145, True) == 16 * 200 * 8 * 65
    assert _lib.min_over_points_backward_scratch_bytes(8, 200, True) == 24 * 200 * 8
    # these values come from the library: tests/test_abi.py compares the header's macro with the exported function
    assert _lib.min_over_points_scratch_bytes(1, 1, 1, False) == 16
    assert _lib.min_over_points_scratch_bytes(3, 7, 4096, True) == 16 * 7 * 3
