"""CPU: the contract of include/pvamd.h "Distance transform" as the brute-force C restatement states it (tests/distance_transform_ref.c)
-- against scipy's exact transform, against a numpy argmin for the tie rule, and on a voxelised ball against the closed form --
plus the declarations, the binding and the argument checks of pv.distance_transform / pv.OccupancySDF, which raise before a GPU
is asked for.  The GPU tests compare the kernels with this restatement bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib, occupancy
from tests import distance_transform_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_GRIDS = (((5, 7, 9), 0.3), ((3, 17, 4), 0.5))
NO_SITE = _lib.EDT_NO_SITE  # the header's PVAMD_EDT_NO_SITE: what the restatement must report for an empty site class


def test_exports_header_and_binding():
    assert pv.DistanceTransform._fields == ("values", "gradients", "sites", "squared")
    for name in ("distance_transform", "OccupancySDF", "cached_sdf_from_voxels"):
        assert callable(getattr(pv, name)), name
    assert issubclass(pv.OccupancySDF, pv.ObjectFrameSDF)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pvamd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+PVAMD_EDT_NO_SITE\s+2147483647\b", text)
    assert re.search(r"\bint64_t\s+pvamd_distance_transform_scratch_bytes\s*\(", text)
    assert re.search(r"\bint\s+pvamd_distance_transform\s*\(", text)
    assert "Distance transform" in open(os.path.join(ROOT, "include", "pvamd.h")).read()
    assert _lib.H["PVAMD_EDT_NO_SITE"] == _lib.EDT_NO_SITE == ref.NO_SITE == 2 ** 31 - 1 and _lib.ABI_VERSION == 16
    c = ctypes
    assert _lib.SIGNATURES["pvamd_distance_transform_scratch_bytes"] == (c.c_int64, [c.c_int32] * 4)
    assert _lib.SIGNATURES["pvamd_distance_transform"] == (c.c_int, [c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_float, c.c_int32,
                                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p])
    lib = _lib.load()
    assert hasattr(lib, "pvamd_distance_transform") and hasattr(lib, "pvamd_distance_transform_scratch_bytes")
    assert os.path.exists(os.path.join(ROOT, "pytorch_volumetric_amd", "csrc", "distance_transform.hip"))
    # the lattice limits: defined in the header, read by the binding, used by the module and, below, by the library
    assert _lib.LATTICE_MAX_AXIS == _lib.H["PVAMD_LATTICE_MAX_AXIS"] == occupancy.MAX_AXIS == 2048
    assert _lib.EDT_MIN_AXIS == _lib.H["PVAMD_EDT_MIN_AXIS"] == occupancy.MIN_AXIS == 1
    assert _lib.EDT_MAX_VOXELS == _lib.H["PVAMD_EDT_MAX_VOXELS"] == occupancy.MAX_VOXELS == 2 ** 31 - 1
    for axis in range(3):
        for n, want in ((occupancy.MAX_AXIS + 1, _lib.E_SHAPE), (occupancy.MIN_AXIS - 1, _lib.E_SHAPE),
                        (occupancy.MAX_AXIS, _lib.H["PVAMD_E_NULL"])):  # the shape is tested before the pointers: no GPU is touched
            shape = [occupancy.MIN_AXIS] * 3
            shape[axis] = n
            assert lib.pvamd_distance_transform(None, *shape, 1.0, 1, None, None, None, None, None) == want, shape
            assert (lib.pvamd_distance_transform_scratch_bytes(*shape, 1) > 0) == (want != _lib.E_SHAPE), shape


def test_scratch_size_is_the_library_function_and_refuses_what_the_entry_point_refuses():
    lib = _lib.load()
    for shape in ((5, 7, 9), (1, 1, 1), (2048, 1, 2), (256, 256, 256)):
        for signed in (False, True):
            size = _lib.distance_transform_scratch_bytes(*shape, signed)
            assert size == lib.pvamd_distance_transform_scratch_bytes(*shape, int(signed)) > 0
            assert size % 4 == 0
        assert _lib.distance_transform_scratch_bytes(*shape, True) == 2 * _lib.distance_transform_scratch_bytes(*shape, False)
    for shape in ((0, 4, 4), (4, 2049, 4), (4, 4, -1), (2048, 2048, 2048)):  # the last: more than 2^31 - 1 voxels
        assert lib.pvamd_distance_transform_scratch_bytes(*shape, 1) == 0, shape
    # argument errors of the entry point return before anything is launched or dereferenced
    assert lib.pvamd_distance_transform(None, 4, 2049, 4, 1.0, 1, None, None, None, None, None) == _lib.E_SHAPE
    assert lib.pvamd_distance_transform(None, 2048, 2048, 2048, 1.0, 1, None, None, None, None, None) == _lib.E_SHAPE
    assert lib.pvamd_distance_transform(None, 4, 4, 4, 1.0, 1, None, None, None, None, None) == _lib.H["PVAMD_E_NULL"]


@pytest.mark.parametrize("shape, fraction", TIE_GRIDS + (((23, 19, 37), 0.02), ((9, 2, 130), 0.1)))
def test_restatement_squared_is_scipys_exact_transform(shape, fraction):
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = ref.random_grid(shape, fraction, seed=7)
    assert 0 < occ.sum() < occ.size
    to_occupied = np.rint(ndimage.distance_transform_edt(occ == 0) ** 2).astype(np.int64).reshape(-1)
    to_free = np.rint(ndimage.distance_transform_edt(occ != 0) ** 2).astype(np.int64).reshape(-1)
    flat = occ.reshape(-1) != 0
    _, _, unsigned_sq = ref.transform(occ, 1.0, signed=False)
    assert np.array_equal(unsigned_sq, to_occupied)  # zero on the occupied voxels in both
    _, _, signed_sq = ref.transform(occ, 1.0, signed=True)
    assert np.array_equal(signed_sq, np.where(flat, to_free, to_occupied))


@pytest.mark.parametrize("shape, fraction", TIE_GRIDS)
def test_restatement_sites_are_the_first_flat_minimum_and_ties_are_common(shape, fraction):
    occ = ref.random_grid(shape, fraction, seed=11)
    flat = occ.reshape(-1) != 0
    coords = np.stack(np.unravel_index(np.arange(occ.size), shape), axis=1).astype(np.int64)
    d2 = ((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1)  # [voxel][site], sites in flat order
    big = np.iinfo(np.int64).max
    tied = 0
    for signed in (True, False):
        rec, sites, squared = ref.transform(occ, 0.25, signed=signed)
        to_occupied = np.where(flat[None, :], d2, big)
        to_free = np.where(~flat[None, :], d2, big)
        cost = np.where(flat[:, None], to_free if signed else np.where(np.eye(occ.size, dtype=bool), 0, big), to_occupied)
        want = cost.argmin(axis=1)  # numpy: the first of equal minima
        assert np.array_equal(sites, want)
        assert np.array_equal(squared, cost.min(axis=1))
        if signed:
            tied = ((cost == cost.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean()
        # the float statements on top of (site, squared)
        s = np.sqrt(squared.astype(np.float32))
        r = np.float32(0.25)
        value = r * (s - np.float32(0.5)) if signed else r * s
        assert np.array_equal(rec[:, 0], np.where(flat & signed, -value, value).astype(np.float32))
        away = ((coords - coords[sites]) * np.where(flat, -1, 1)[:, None]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            grad = np.where(squared[:, None] > 0, away / s[:, None], np.float32(0))
        assert np.array_equal(rec[:, 1:], grad.astype(np.float32))
        assert not np.signbit(rec[squared == 0]).any()  # unsigned, occupied: +0.0 and a zero gradient
    assert tied > 0.05, tied  # the tie rule is exercised


def test_restatement_sentinels():
    for fill, sign in ((0, 1.0), (1, -1.0)):
        rec, sites, squared = ref.transform(np.full((3, 4, 5), fill, np.uint8), 0.5, signed=True)
        assert (squared == NO_SITE).all() and (sites == -1).all()
        assert (rec[:, 0] == sign * np.inf).all() and (rec[:, 1:] == 0).all()
    rec, sites, squared = ref.transform(np.ones((3, 4, 5), np.uint8), 0.5, signed=False)
    assert (squared == 0).all() and np.array_equal(sites, np.arange(60)) and (rec == 0).all()


def test_restatement_on_a_voxelised_ball_follows_the_closed_form():
    """A voxel centre lies within (sqrt(3) / 2) res of any point, and the surface of the field lies on voxel faces: for a free voxel
    -0.5 res <= value - (|c| - r) <= (sqrt(3) - 0.5) res, mirrored for an occupied one."""
    occ, norm = ref.ball()
    assert occ.shape == (51, 51, 51)
    res, eps = ref.BALL_RES, 1e-5
    rec, sites, squared = ref.transform(occ, res, signed=True)
    flat = occ.reshape(-1) != 0
    err = rec[:, 0].astype(np.float64) - (norm.reshape(-1) - ref.BALL_RADIUS)
    lo, hi = -0.5 * res - eps, (np.sqrt(3) - 0.5) * res + eps
    print(f"ball: free err in [{err[~flat].min():.5f}, {err[~flat].max():.5f}], occupied err in [{err[flat].min():.5f}, "
          f"{err[flat].max():.5f}], allowed [{lo:.5f}, {hi:.5f}] / mirrored")
    assert (err[~flat] >= lo).all() and (err[~flat] <= hi).all()
    assert (err[flat] >= -hi).all() and (err[flat] <= -lo).all()
    c = ref.ball_centres()
    radial = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    assert ((rec[:, 1:].astype(np.float64) * radial).sum(-1)[~flat] > 0).all()


def test_argument_errors_are_raised_without_a_gpu():
    ok = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for bad in (torch.zeros((4, 5)), torch.zeros((2, 3, 4, 5)), torch.zeros((3, 0, 5)), torch.zeros((1, 2049, 1), dtype=torch.bool)):
        with pytest.raises(ValueError):
            pv.distance_transform(bad)
    for resolution in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            pv.distance_transform(ok, resolution=resolution)
    for signed in (1, 0, None, "yes"):
        with pytest.raises(TypeError):
            pv.distance_transform(ok, signed=signed)
    planar = pv.VoxelGrid(0.1, [(0.0, 1.0), (0.0, 1.0)])
    with pytest.raises(ValueError):
        pv.OccupancySDF(planar)
    with pytest.raises(TypeError):
        pv.OccupancySDF(pv.VoxelGrid(0.1, [(0.0, 1.0)] * 3), signed=1)
