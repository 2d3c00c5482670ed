"""Restatement of the redistancing contract (include/pvamd.h "Redistancing") for its tests -- TEST INFRASTRUCTURE:
redistance_ref.c compiled on the fly (the nested separable form, which is the definition, and a brute force over every
crossing), and the fields the CPU and GPU tests share."""
import ctypes
import functools

import numpy as np

from tests import c_ref

KEPT = -2


def load():
    lib = c_ref.load("redistance_ref")
    lib.redistance_ref.restype = ctypes.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def as_records(values, gradients=None):
    """(nx, ny, nz, 4) float32 records from values and optional (nx, ny, nz, 3) gradients (zeros without)."""
    values = np.asarray(values, np.float32)
    rec = np.zeros(values.shape + (4,), np.float32)
    rec[..., 0] = values
    if gradients is not None:
        rec[..., 1:] = gradients
    return rec


def redistance(records, resolution=1.0, band=0.0, max_distance=np.inf):
    """(records (n, 4) float32, sites (n,) int32, squared (n,) float32) of (nx, ny, nz, 4) float32 records: the nested form."""
    assert records.dtype == np.float32 and records.flags.c_contiguous and records.ndim == 4 and records.shape[3] == 4
    nx, ny, nz = records.shape[:3]
    n = nx * ny * nz
    out = np.empty((n, 4), np.float32)
    sites = np.empty((n,), np.int32)
    squared = np.empty((n,), np.float32)
    f = ctypes.c_float
    differ = load().redistance_ref(_p(records), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), f(resolution), f(band),
                                   f(max_distance), _p(out), _p(sites), _p(squared))
    assert differ == 0, f"the nested cost differs from statement 3 at its own site at {differ} voxels"
    return out, sites, squared


def brute(records):
    """(n,) float32: the minimum of c3 over every crossing of the lattice, +inf without one."""
    assert records.dtype == np.float32 and records.flags.c_contiguous
    nx, ny, nz = records.shape[:3]
    squared = np.empty((nx * ny * nz,), np.float32)
    load().redistance_brute(_p(records), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), _p(squared))
    return squared


def site_costs(records, sites):
    """(n,) float32: c3 of the crossing each site names, seen from its voxel; +inf where sites < 0 or the edge has no crossing."""
    assert records.dtype == np.float32 and records.flags.c_contiguous and sites.dtype == np.int32
    nx, ny, nz = records.shape[:3]
    out = np.empty((nx * ny * nz,), np.float32)
    load().redistance_site_costs(_p(records), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), _p(sites), _p(out))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------- the fields the tests share
@functools.lru_cache(maxsize=None)
def smooth_field(shape, seed=5):
    """(nx, ny, nz, 4) float32 records, read-only: a few waves plus noise, many crossings of every family at generic fractions;
    the gradient columns hold noise of their own, so that a kept record is recognisable."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    values = np.sin(0.9 * x + 0.3) * np.cos(0.7 * y) + 0.8 * np.sin(0.23 * z + 0.5 * x) + 0.3 * rng.standard_normal(shape)
    values -= np.median(values)  # both signs on any lattice, (2, 2, 2) included
    rec = as_records(values, rng.standard_normal(shape + (3,)))
    rec.flags.writeable = False
    return rec


@functools.lru_cache(maxsize=None)
def tie_field(shape):
    """(nx, ny, nz, 4) float32 records, read-only: the integer-valued x^2 + y^2 + z^2 - c about the lattice's centre (doubled
    coordinates, so that even axes are centred too): symmetric, so equal costs abound within and across the families."""
    axes = [2.0 * np.arange(s) - (s - 1) for s in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    r2 = x * x + y * y + z * z
    values = r2 - np.floor(0.35 * r2.max())
    if not ((values < 0).any() and (values >= 0).any()):
        values = x + y + z + 1.0  # (2, 2, 2), where every r2 is 3: a plane through the lattice instead
    rec = as_records(values, np.ones(shape + (3,)))
    rec.flags.writeable = False
    return rec


@functools.lru_cache(maxsize=None)
def half_field(shape):
    """(nx, ny, nz, 4) float32 records, read-only: +1 up to the middle of x, -1 beyond it.  The only crossings sit at f = 0.5
    exactly, so the voxels three slabs to either side of them are exactly 3.5 voxels away, squared == 12.25: whether they keep
    their site under max_distance = 3.5 * resolution turns on the rounding of max_distance / resolution and of Rv * Rv."""
    values = np.ones(shape)
    values[shape[0] // 2 + 1:] = -1.0
    rec = as_records(values, np.ones(shape + (3,)))
    rec.flags.writeable = False
    return rec


FIELDS = {"smooth": smooth_field, "tie": tie_field, "half": half_field}
ROUNDING_RESOLUTIONS = (0.013, 0.02, 0.037)  # max_distance / resolution of 3.5 * resolution: below 3.5 under the first only

TINY = (1e-39, -1e-39, 1.4e-45, -1.4e-45, 0.0, -0.0)  # denormals of either sign, the smallest ones, and both zeros


@functools.lru_cache(maxsize=None)
def tiny_field(shape, seed=9):
    """((nx, ny, nz, 4) float32 records, (nx, ny, nz) bool: which samples were replaced), read-only: smooth_field with about 1 %
    of its samples replaced, in a seeded pattern, by TINY: the samples for which f = V_a / (V_a - V_b) has a denormal numerator
    or denominator, and for which (V_a < 0) == (V_b < 0) turns on the sign of zero."""
    rec = smooth_field(shape).copy()
    kind = np.random.default_rng(seed).integers(0, 100 * len(TINY), size=shape)
    for code, value in enumerate(TINY):
        rec[..., 0][kind == code] = np.float32(value)
    rec.flags.writeable = False
    return rec, kind < len(TINY)


@functools.lru_cache(maxsize=None)
def one_negative_field(shape, far, seed=13):
    """(nx, ny, nz, 4) float32 records, read-only: positive noise everywhere but one negative voxel, the far corner
    (n - 1 on every axis) or voxel (0, 0, 0): the lattice's only crossings are on the three edges that leave it."""
    values = np.random.default_rng(seed).uniform(0.5, 1.5, size=shape)
    values[tuple(s - 1 for s in shape) if far else (0, 0, 0)] = -0.7
    rec = as_records(values)
    rec.flags.writeable = False
    return rec

BALL_RADIUS, BALL_RES, BALL_BAND = 0.3, 0.02, 0.06  # the band: 3 voxels


def ball_values(centre=(0.0, 0.0, 0.0)):
    """(values (51, 51, 51) float32 clipped to +/-BALL_BAND, exact signed distance float64) of a ball of BALL_RADIUS about
    `centre` on the 51^3 lattice over [-0.5, 0.5]^3."""
    c = np.linspace(-0.5, 0.5, 51)
    x, y, z = np.meshgrid(c - centre[0], c - centre[1], c - centre[2], indexing="ij")
    exact = np.sqrt(x * x + y * y + z * z) - BALL_RADIUS
    return np.clip(exact, -BALL_BAND, BALL_BAND).astype(np.float32), exact
