"""CPU: the interpolation= keyword of CachedSDF (validation, plan invalidation) and a self-check of the trilinear restatement
(tests/interp_ref.c) on grids where the exact answer is known."""
import inspect

import numpy as np
import pytest

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import interp_ref as R


def test_default_is_nearest_and_trails_the_reference_parameters():
    params = list(inspect.signature(pv.CachedSDF.__init__).parameters.values())
    assert params[-1].name == "interpolation" and params[-1].default == "nearest"
    assert params[-2].name == "cache_path"


@pytest.mark.parametrize("bad", ["linear", "Trilinear", None, 1])
def test_unknown_interpolation_raises(bad):
    with pytest.raises(ValueError, match="interpolation"):
        pv.CachedSDF("x", 0.1, [(0.0, 1.0)] * 3, None, cache_path=None, interpolation=bad)


def test_planar_trilinear_raises():
    with pytest.raises(ValueError, match="3-D"):
        pv.CachedSDF("x", 0.1, [(0.0, 1.0)] * 2, None, cache_path=None, interpolation="trilinear")


def test_setting_the_attribute_invalidates_plans_and_is_validated():
    assert "interpolation" in pv.CachedSDF._PLAN_ATTRS
    c = object.__new__(pv.CachedSDF)
    c.__dict__["_dim"] = 3
    before = _lib.EPOCH[0]
    c.interpolation = "trilinear"
    assert _lib.EPOCH[0] > before and c.interpolation == "trilinear"
    with pytest.raises(ValueError):
        c.interpolation = "cubic"
    c.__dict__["_dim"] = 2
    with pytest.raises(ValueError):
        c.interpolation = "trilinear"


def dyadic_grid(shape, mn, res, coef):
    """Records that are an affine function of the voxel centre: val = c0 + c . x, gradient = (c1, c2, c3) + position terms."""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    x = mn + idx * res
    rec = np.empty((x.shape[0], 4), np.float32)
    for q in range(4):
        rec[:, q] = coef[q, 0] + x @ coef[q, 1:]
    return rec


def affine(coef, x):
    return np.stack([coef[q, 0] + x @ coef[q, 1:] for q in range(4)], -1)


@pytest.mark.parametrize("f64", [False, True])
def test_restatement_is_exact_on_affine_records(f64):
    shape = np.array([5, 6, 7], np.int32)
    mn = np.array([-1.0, 0.5, -0.25])
    res = np.array([0.25, 0.5, 0.125])
    rng = np.random.default_rng(0)
    coef = rng.integers(-8, 9, size=(4, 4)) / 4.0
    rec = dyadic_grid(shape, mn, res, coef)
    dt = np.float64 if f64 else np.float32
    hi = mn + (shape - 1) * res
    # dyadic points on a 1/64-voxel lattice inside the range: every step of the contract is exact
    k = rng.integers(0, 64 * (shape - 1) + 1, size=(2000, 3))
    pts = (mn + k * res / 64).astype(dt)
    assert np.all(pts >= mn) and np.all(pts <= hi)
    val, grad = R.forward(rec, shape, mn.astype(dt), res.astype(dt), pts, np.ones(len(pts), bool))
    want = affine(coef, pts.astype(np.float64))
    assert np.array_equal(val, want[:, 0].astype(dt)) and np.array_equal(grad, want[:, 1:].astype(dt))
    # the VJP of an affine interpolant is its slope (divided back from the fraction): d val / dx = coef[0, 1:]
    inner = np.all((k > 0) & (k < 64 * (shape - 1)), axis=1)
    d = R.vjp(rec, shape, mn, res, pts.astype(np.float64), inner, np.ones(len(pts)), np.zeros((len(pts), 3)))
    assert np.allclose(d[inner], coef[0, 1:], rtol=0, atol=1e-12)


@pytest.mark.parametrize("f64", [False, True])
def test_restatement_returns_records_at_voxel_centres(f64):
    shape = np.array([4, 3, 5], np.int32)
    mn = np.array([0.5, -2.0, 1.0])
    res = np.array([0.5, 0.25, 1.0])
    rng = np.random.default_rng(1)
    rec = (rng.integers(-64, 65, size=(int(np.prod(shape)), 4)) / 8.0).astype(np.float32)
    dt = np.float64 if f64 else np.float32
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    pts = (mn + idx * res).astype(dt)
    val, grad = R.forward(rec, shape, mn.astype(dt), res.astype(dt), pts, np.ones(len(pts), bool))
    assert np.array_equal(val, rec[:, 0].astype(dt)) and np.array_equal(grad, rec[:, 1:].astype(dt))
