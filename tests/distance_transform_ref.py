"""Restatement of the distance-transform contract (include/pvamd.h "Distance transform") for its tests -- TEST INFRASTRUCTURE:
distance_transform_ref.c compiled on the fly (the O(n * |Q|) brute force with the contract's float statements), and the grids
the CPU and GPU tests share."""
import ctypes
import functools

import numpy as np

from tests import c_ref

NO_SITE = 2 ** 31 - 1


def load():
    return c_ref.load("distance_transform_ref")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def transform(occ, resolution=1.0, signed=True):
    """(records (n, 4) float32, sites (n,) int32, squared (n,) int32) of a 3-D occupancy array (non-zero = occupied)."""
    occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
    nx, ny, nz = occ.shape
    n = occ.size
    records = np.empty((n, 4), np.float32)
    sites = np.empty((n,), np.int32)
    squared = np.empty((n,), np.int32)
    load().edt_ref(_p(occ), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), ctypes.c_float(resolution),
                   ctypes.c_int32(int(signed)), _p(records), _p(sites), _p(squared))
    return records, sites, squared


def random_grid(shape, fraction, seed):
    """uint8 occupancy with about `fraction` of the voxels occupied."""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < fraction).astype(np.uint8)


BALL_RADIUS, BALL_RES = 0.3, 0.02
BALL_RANGE = [(-0.5, 0.5)] * 3


def ball_centres():
    """Voxel-centre coordinates per axis of the ball's lattice: 51 float64 values over [-0.5, 0.5]."""
    return np.linspace(-0.5, 0.5, 51)


@functools.lru_cache(maxsize=1)
def ball():
    """(occupancy (51, 51, 51) uint8, centre norms (51, 51, 51) float64) of the voxelised ball |c| <= BALL_RADIUS."""
    c = ball_centres()
    norm = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return (norm <= BALL_RADIUS).astype(np.uint8), norm
