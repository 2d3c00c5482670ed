"""Redistancing without a GPU: the argument errors of pv.redistance and of the far_field keywords, the binding, and the properties
the contract's statements (include/pvamd.h "Redistancing") must have, checked on their C restatement (tests/redistance_ref.c)."""
import functools
import math
import sys

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import distance_transform_ref as edt_ref
from tests import redistance_ref as ref
from tests import tsdf_ref

redistance_module = sys.modules["pytorch_volumetric_amd.redistance"]  # the package's attribute of that name is the function

INF = np.float32(np.inf)


# ---------------------------------------------------------------- the Python layer
def test_the_entry_points_reach_the_binding():
    assert len(_lib.SIGNATURES["pvamd_redistance"][1]) == 12 and len(_lib.SIGNATURES["pvamd_redistance_scratch_bytes"][1]) == 3
    assert _lib.ABI_VERSION == 16 and _lib.REDIST_KEPT == ref.KEPT == -2
    assert pv.redistance is redistance_module.redistance and pv.Redistance is redistance_module.Redistance
    assert pv.Redistance._fields == ("values", "gradients", "sites", "squared")
    # the lattice limits: defined in the header, read by the binding, used by the module and, below, by the library
    MIN, MAX = redistance_module.MIN_AXIS, redistance_module.MAX_AXIS
    assert _lib.LATTICE_MAX_AXIS == _lib.H["PVAMD_LATTICE_MAX_AXIS"] == MAX == 2048
    assert _lib.REDIST_MIN_AXIS == _lib.H["PVAMD_REDIST_MIN_AXIS"] == MIN == 2
    assert _lib.REDIST_MAX_VOXELS == _lib.H["PVAMD_REDIST_MAX_VOXELS"] == redistance_module.MAX_VOXELS == 2 ** 29
    lib = _lib.load()
    for axis in range(3):
        for n, want in ((MAX + 1, _lib.E_SHAPE), (MIN - 1, _lib.E_SHAPE), (MAX, _lib.H["PVAMD_E_NULL"])):
            shape = [MIN] * 3  # the shape is tested before the pointers: no GPU is touched
            shape[axis] = n
            assert lib.pvamd_redistance(None, *shape, 1.0, 0.0, 1.0, None, None, None, None, None) == want, shape
            assert (lib.pvamd_redistance_scratch_bytes(*shape) > 0) == (want != _lib.E_SHAPE), shape


VALUES = torch.ones(3, 4, 5)


@pytest.mark.parametrize("error, args, kwargs", [
    (ValueError, (torch.ones(4, 5),), {}),                                     # not 3-D
    (ValueError, (torch.ones(2, 3, 4, 5),), {}),
    (ValueError, (torch.ones(1, 4, 5),), {}),                                  # an axis of one voxel
    (ValueError, (torch.ones(1, 1, 1).expand(2, 2, 2049),), {}),               # an axis too long
    (ValueError, (torch.ones(1, 1, 1).expand(1024, 1024, 513),), {}),          # more than 2^29 voxels
    (TypeError, (torch.ones(3, 4, 5, dtype=torch.complex64),), {}),
    (ValueError, (VALUES,), dict(resolution=0.0)),
    (ValueError, (VALUES,), dict(resolution=-1.0)),
    (ValueError, (VALUES,), dict(resolution=math.nan)),
    (ValueError, (VALUES,), dict(resolution=math.inf)),
    (TypeError, (VALUES,), dict(resolution="1")),
    (ValueError, (VALUES,), dict(band=-0.5, gradients=torch.zeros(3, 4, 5, 3))),
    (ValueError, (VALUES,), dict(band=math.nan, gradients=torch.zeros(3, 4, 5, 3))),
    (TypeError, (VALUES,), dict(band=None)),
    (TypeError, (VALUES,), dict(band=True)),
    (ValueError, (VALUES,), dict(band=0.5)),                                   # kept voxels need their gradients
    (ValueError, (VALUES,), dict(band=0.5, gradients=torch.zeros(3, 4, 5))),
    (ValueError, (VALUES,), dict(gradients=torch.zeros(3, 4, 4, 3))),
    (TypeError, (VALUES,), dict(gradients=torch.zeros(3, 4, 5, 3, dtype=torch.complex64))),
    (ValueError, (VALUES,), dict(max_distance=0.0)),
    (ValueError, (VALUES,), dict(max_distance=-1.0)),
    (ValueError, (VALUES,), dict(max_distance=math.nan)),
    (TypeError, (VALUES,), dict(max_distance="far")),
])
def test_argument_errors_are_raised_before_a_gpu_is_asked_for(error, args, kwargs, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    with pytest.raises(error):
        pv.redistance(*args, **kwargs)


def test_the_far_field_keywords_are_checked_before_a_gpu_is_asked_for(monkeypatch):
    volume = pv.TSDFVolume(0.25, [(-1.0, 1.0), (-1.0, 1.0), (0.0, 1.5)], truncation=0.75, device="cpu")
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    for far_field in (1, 0, "yes", None):
        with pytest.raises(TypeError):
            pv.TSDFField(volume, far_field=far_field)
        with pytest.raises(TypeError):
            volume.to_sdf("scene", far_field=far_field)
    for kwargs in (dict(max_distance=0.5), dict(far_field=False, max_distance=2.0), dict(far_field=True, max_distance=0.0),
                   dict(far_field=True, max_distance=-1.0), dict(far_field=True, max_distance=math.nan)):
        with pytest.raises(ValueError):
            pv.TSDFField(volume, **kwargs)
        with pytest.raises(ValueError):
            volume.to_sdf("scene", **kwargs)
    with pytest.raises(TypeError):
        pv.TSDFField(volume, far_field=True, max_distance="far")
    with pytest.raises(_lib.PvamdError):  # the arguments are fine: a volume in host memory has no kernel
        pv.TSDFField(volume, far_field=True, max_distance=0.5)


# ---------------------------------------------------------------- the statements, on their restatement
FIELDS = [("smooth", (6, 5, 7)), ("tie", (6, 5, 7)), ("tie", (7, 7, 7)), ("smooth", (2, 2, 2)), ("tie", (2, 2, 2))]


@pytest.mark.parametrize("field, shape", FIELDS)
def test_the_nested_form_is_the_minimum_over_all_crossings_and_its_site_attains_it(field, shape):
    rec = ref.FIELDS[field](shape)
    out, sites, squared = ref.redistance(rec)
    want = ref.brute(rec)
    assert np.isfinite(want).all()  # every field here has a crossing
    assert np.array_equal(ref.bits(squared), ref.bits(want)), int((ref.bits(squared) != ref.bits(want)).sum())
    assert (sites >= 0).all() and np.array_equal(ref.bits(ref.site_costs(rec, sites)), ref.bits(squared))
    families = np.bincount(sites & 3, minlength=3)
    assert shape == (2, 2, 2) or (families > 0).all()
    # values and gradients follow from (site, squared)
    values = rec[..., 0].reshape(-1)
    assert np.array_equal(out[:, 0], np.where(values < 0, -np.sqrt(squared), np.sqrt(squared)))
    length = np.linalg.norm(out[:, 1:].astype(np.float64), axis=1)
    assert (np.abs(length[squared > 0] - 1) < 1e-6).all() and not out[squared == 0, 1:].any()


def test_ties_abound_in_the_tie_field_and_the_lower_family_and_coordinate_win():
    rec = ref.tie_field((7, 7, 7))
    assert np.array_equal(rec[..., 0], np.round(rec[..., 0]))  # integer valued
    _, sites, squared = ref.redistance(rec)
    sq, st = squared.reshape(7, 7, 7), sites.reshape(7, 7, 7)
    # the field is symmetric under every permutation of the axes, and so are the squared distances, bit for bit; under a
    # reflection f becomes 1 - f, which rounds differently
    for axes in ((1, 0, 2), (2, 1, 0), (0, 2, 1)):
        assert np.array_equal(sq, sq.transpose(axes))
    for axis in range(3):
        assert np.allclose(sq, np.flip(sq, axis), rtol=1e-6, atol=0)
    # the centre is equally far from the images of its nearest crossing under all 48 symmetries: family x wins, and in it the
    # edge with the lower coordinate on every axis
    centre = st[3, 3, 3]
    a = np.unravel_index(centre >> 2, (7, 7, 7))
    assert centre & 3 == 0 and a[0] < 3 and a[1] <= 3 and a[2] <= 3


def test_kept_voxels_are_bit_copies_and_the_others_do_not_depend_on_the_band():
    rec = ref.smooth_field((6, 5, 7)).copy()
    rec[0, 0, 0] = (-0.0, -0.0, np.nan, 7.0)  # |-0.0| < band: kept, whatever its gradient holds
    free, free_sites, free_squared = ref.redistance(rec)
    out, sites, squared = ref.redistance(rec, band=0.5)
    flat = rec.reshape(-1, 4)
    kept = np.abs(flat[:, 0]) < 0.5
    assert 20 < kept.sum() < kept.size - 20 and kept[0]
    assert np.array_equal(ref.bits(out[kept]), ref.bits(flat[kept]))
    assert (sites[kept] == ref.KEPT).all() and (squared[kept] == INF).all()
    assert np.array_equal(ref.bits(out[~kept]), ref.bits(free[~kept])) and np.array_equal(sites[~kept], free_sites[~kept])
    assert np.array_equal(ref.bits(squared[~kept]), ref.bits(free_squared[~kept]))
    everything = ref.redistance(rec, band=np.inf)  # every finite sample is inside an infinite band
    assert np.array_equal(ref.bits(everything[0]), ref.bits(flat)) and (everything[1] == ref.KEPT).all()


def test_max_distance_cuts_the_field_and_a_field_without_crossings_is_far_everywhere():
    rec = ref.smooth_field((19, 13, 37))
    free, free_sites, free_squared = ref.redistance(rec, resolution=0.5)
    out, sites, squared = ref.redistance(rec, resolution=0.5, max_distance=0.75)  # 1.5 voxels: R2 = 2.25
    far = free_squared > 2.25
    assert 100 < far.sum() < far.size - 100
    negative = rec[..., 0].reshape(-1) < 0
    assert (sites[far] == -1).all() and (squared[far] == INF).all() and not out[far, 1:].any()
    assert np.array_equal(out[far, 0], np.where(negative[far], np.float32(-0.75), np.float32(0.75)))
    assert np.array_equal(ref.bits(out[~far]), ref.bits(free[~far])) and np.array_equal(sites[~far], free_sites[~far])
    assert np.abs(out[:, 0]).max() == 0.75
    for values in (np.full((3, 4, 5), 2.0, np.float32), np.full((3, 4, 5), -2.0, np.float32)):
        for max_distance in (np.inf, 1.5):
            out, sites, squared = ref.redistance(ref.as_records(values), max_distance=max_distance)
            assert (sites == -1).all() and (squared == INF).all() and not out[:, 1:].any()
            assert (out[:, 0] == np.float32(math.copysign(max_distance, values[0, 0, 0]))).all()


def test_edges_with_a_nan_or_infinite_endpoint_carry_no_crossing():
    values = np.ones((4, 3, 5), np.float32)
    values[0] = -1.0
    values[1] = np.nan  # the only sign change of the lattice runs through NaN samples: no crossing at all
    out, sites, squared = ref.redistance(ref.as_records(values))
    assert (sites == -1).all() and (squared == INF).all()
    assert np.array_equal(out[:, 0], np.where(values.reshape(-1) < 0, -INF, INF))  # NaN counts as not negative
    values[1] = -np.inf
    assert (ref.redistance(ref.as_records(values))[1] == -1).all()
    values[1, 1, 2] = -3.0  # one finite sample in the slab: of its six edges only the one toward x = 2 has two finite ends of
    #                         different sign: the lattice's one crossing, family x at (1, 1, 2)
    rec = ref.as_records(values)
    out, sites, squared = ref.redistance(rec)
    assert np.array_equal(ref.bits(squared), ref.bits(ref.brute(rec))) and (sites >= 0).all()
    lower, axis = np.unravel_index(sites >> 2, values.shape), sites & 3
    upper = tuple(lower[k] + (axis == k) for k in range(3))
    assert np.isfinite(values[lower]).all() and np.isfinite(values[upper]).all()
    assert (sites == ((1 * 3 + 1) * 5 + 2) * 4 + 0).all()
    # noise with NaN and infinities sprinkled in: still the minimum over the crossings that remain
    rec = ref.smooth_field((6, 5, 7)).copy()
    kind = np.random.default_rng(1).integers(0, 12, size=(6, 5, 7))
    for code, bad in enumerate((np.nan, np.inf, -np.inf)):
        rec[..., 0][kind == code] = bad
    out, sites, squared = ref.redistance(rec, band=0.25)
    kept = np.abs(rec[..., 0].reshape(-1)) < 0.25
    assert not kept[np.isnan(rec[..., 0].reshape(-1))].any()  # a NaN sample is never kept
    assert np.array_equal(ref.bits(squared[~kept]), ref.bits(ref.brute(rec)[~kept]))
    assert np.isnan(rec[..., 0]).sum() > 5 and np.isfinite(squared[~kept]).all()


# ---------------------------------------------------------------- accuracy: what the feature is for
def errors_in_voxels(values, exact, res, band):
    """(mean, worst) absolute error in voxels of `values` against `exact` over the voxels outside the band."""
    outside = np.abs(exact) >= band
    err = np.abs(values.astype(np.float64) - exact)[outside] / res
    return err.mean(), err.max()


def both_routes(values, res, band):
    """(redistanced values, occupancy-route values) of a clipped field, float32 (nx, ny, nz)."""
    far = ref.redistance(ref.as_records(values), resolution=res)[0][:, 0].reshape(values.shape)
    occ = edt_ref.transform(values < 0, resolution=res, signed=True)[0][:, 0].reshape(values.shape)
    return far, occ


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (0.0071, -0.0043, 0.0113)])
def test_a_ball_from_clipped_analytic_values_is_far_closer_than_the_occupancy_route(centre):
    """51^3 at 0.02, radius 0.3, values clipped to +/-3 voxels; outside that band, against |c| - r.  Measured here, in voxels:
    centred 0.0165 mean / 0.112 worst against 0.267 / 0.500 by the occupancy route; off-centre 0.0160 / 0.103 against
    0.305 / 0.499."""
    values, exact = ref.ball_values(centre)
    far, occ = both_routes(values, ref.BALL_RES, ref.BALL_BAND)
    mean, worst = errors_in_voxels(far, exact, ref.BALL_RES, ref.BALL_BAND)
    occ_mean, occ_worst = errors_in_voxels(occ, exact, ref.BALL_RES, ref.BALL_BAND)
    print(f"centre {centre}: redistanced mean {mean:.4f} worst {worst:.4f}; occupancy route mean {occ_mean:.4f} worst {occ_worst:.4f}")
    assert mean <= 0.25 * occ_mean
    assert worst < occ_worst


@functools.lru_cache(maxsize=None)
def fused_ball():
    """The six-view ball of tests/test_tsdf.py: (records (51, 51, 51, 4) of the fused volume, unknown free; exact distance)."""
    lat = tsdf_ref.make_lattice((51, 51, 51), (-0.5, -0.5, -0.5), ref.BALL_RES)
    intrinsics = (150.0, 150.0, 79.5, 59.5)
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, intrinsics, 120, 160, (0.0, 0.0, 0.0), ref.BALL_RADIUS)
    state = np.zeros(lat.dims + (2,), np.float32)
    tsdf_ref.integrate(lat, state, depth, tsdf_ref.invert(poses), intrinsics, ref.BALL_BAND)
    rec = tsdf_ref.records(state, ref.BALL_RES, ref.BALL_BAND).reshape(lat.dims + (4,))
    exact = np.linalg.norm(tsdf_ref.centres(lat).astype(np.float64), axis=-1) - ref.BALL_RADIUS
    rec.flags.writeable = False
    return rec, exact


def test_a_ball_fused_from_six_views_is_closer_than_the_occupancy_route():
    """The same comparison on a volume fused from six views, band = truncation, unknown space free.  No view sees the core of
    the ball, which therefore reads as free in both routes, 27 voxels wrong at worst in either: the mean over everything outside
    the band is asserted as it stands, and again over the voxels outside the ball, where the routes differ.  Measured here, in
    voxels: everything outside the band 0.680 mean / 26.5 worst against 0.898 / 26.5 by the occupancy route; outside the ball
    0.103 / 0.570 against 0.340 / 0.664."""
    rec, exact = fused_ball()
    out = ref.redistance(rec, resolution=ref.BALL_RES, band=ref.BALL_BAND)[0].reshape(rec.shape)
    occ = edt_ref.transform(rec[..., 0] < 0, resolution=ref.BALL_RES, signed=True)[0][:, 0].reshape(exact.shape)
    mean, worst = errors_in_voxels(out[..., 0], exact, ref.BALL_RES, ref.BALL_BAND)
    occ_mean, occ_worst = errors_in_voxels(occ, exact, ref.BALL_RES, ref.BALL_BAND)
    print(f"fused: redistanced mean {mean:.4f} worst {worst:.4f}; occupancy route mean {occ_mean:.4f} worst {occ_worst:.4f}")
    assert mean < occ_mean
    exterior = np.where(exact > 0, exact, 0.0)  # zero inside the ball: inside the band, so left out
    mean, worst = errors_in_voxels(out[..., 0], exterior, ref.BALL_RES, ref.BALL_BAND)
    occ_mean, occ_worst = errors_in_voxels(occ, exterior, ref.BALL_RES, ref.BALL_BAND)
    print(f"fused, outside the ball: redistanced mean {mean:.4f} worst {worst:.4f}; occupancy route mean {occ_mean:.4f} worst {occ_worst:.4f}")
    assert mean < occ_mean
    # kept voxels are the volume's records, and the redistanced ones have unit gradients that point out of the ball outside it
    kept = np.abs(rec[..., 0]) < np.float32(ref.BALL_BAND)
    assert 5000 < kept.sum() and np.array_equal(ref.bits(out[kept]), ref.bits(rec[kept]))
    outside = (exact > ref.BALL_BAND) & ~kept
    c = tsdf_ref.centres(tsdf_ref.make_lattice((51, 51, 51), (-0.5, -0.5, -0.5), ref.BALL_RES)).astype(np.float64)
    cosine = (out[..., 1:][outside] * c[outside]).sum(-1) / np.linalg.norm(c[outside], axis=-1)
    assert outside.sum() > 50000 and cosine.min() > 0 and cosine.mean() > 0.99
    assert (np.sign(out[..., 0]) == np.sign(rec[..., 0])).all()  # signs are kept: the bounding box does not move
