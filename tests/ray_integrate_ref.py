"""Restatement of the ray-integration contract (include/pvamd.h "Ray integration") for its tests -- TEST INFRASTRUCTURE:
ray_integrate_ref.c compiled on the fly, the lattices and the ray sets the CPU and GPU tests share."""
import ctypes

import numpy as np

from tests import c_ref

MARK_FREE, MARK_HIT = 1, 2


class Lattice(ctypes.Structure):
    """lattice_t of ray_integrate_ref.c: the fields of pvamd_grid_t the contract reads."""
    _fields_ = [("dmin", ctypes.c_double * 3), ("dmax", ctypes.c_double * 3), ("dres", ctypes.c_double * 3),
                ("fmin", ctypes.c_float * 3), ("fmax", ctypes.c_float * 3), ("fres", ctypes.c_float * 3),
                ("shape", ctypes.c_int32 * 3), ("index_f64", ctypes.c_int32), ("rule", ctypes.c_int32)]

    @property
    def dims(self):
        return tuple(self.shape)


def load():
    lib = c_ref.load("ray_integrate_ref")
    lib.ray_walk_ref.restype = ctypes.c_int32
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lattice_of(desc):
    """Lattice from anything with pvamd_grid_t's fields (a _lib.GridDesc)."""
    lat = Lattice()
    for name, _ in Lattice._fields_:
        value = getattr(desc, name)
        if name in ("index_f64", "rule"):
            setattr(lat, name, value)
        else:
            for k in range(3):
                getattr(lat, name)[k] = value[k]
    return lat


def unit_lattice(shape, lo=(0.0, 0.0, 0.0), res=1.0):
    """A float32-indexed lattice whose voxel i of axis k is centred on lo_k + i * res: no library needed."""
    lat = Lattice()
    for k in range(3):
        fmin, fres = np.float32(lo[k]), np.float32(res)
        fmax = np.float32(fmin + np.float32(shape[k] - 1) * fres)
        lat.fmin[k], lat.fmax[k], lat.fres[k] = fmin, fmax, fres
        lat.dmin[k], lat.dmax[k], lat.dres[k] = float(fmin), float(fmax), float(fres)
        lat.shape[k] = shape[k]
    return lat


def walk(lat, origin, endpoint, max_range=np.inf):
    """The cells one ray visits, in order, as an (m, 3) int array of voxel indices."""
    nx, ny, nz = lat.dims
    cells = np.empty((nx + ny + nz,), np.int64)
    o = np.ascontiguousarray(origin, np.float32)
    e = np.ascontiguousarray(endpoint, np.float32)
    count = load().ray_walk_ref(ctypes.byref(lat), _p(o), _p(e), ctypes.c_float(max_range), _p(cells))
    return np.stack(np.unravel_index(cells[:count], (nx, ny, nz)), axis=1).reshape(-1, 3)


def mark(lat, origins, endpoints, max_range=np.inf, marks=None):
    """uint8 (nx, ny, nz) marks of one scan; origins (3,) or (1, 3): shared, else (R, 3).  `marks`: accumulate into these."""
    nx, ny, nz = lat.dims
    e = np.ascontiguousarray(endpoints, np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    shared = o.shape[0] == 1 and e.shape[0] != 1
    assert shared or o.shape == e.shape
    marks = np.zeros((nx, ny, nz), np.uint8) if marks is None else marks
    cells = np.empty((nx + ny + nz,), np.int64)
    load().ray_mark_ref(ctypes.byref(lat), _p(o), ctypes.c_int32(int(shared)), _p(e), ctypes.c_int64(e.shape[0]),
                        ctypes.c_float(max_range), _p(marks), _p(cells))
    return marks


def update(marks, log_odds, observed, l_hit, l_miss, l_min, l_max):
    """Statement 8 in place on contiguous numpy arrays (uint8, float32, uint8)."""
    load().occupancy_update_ref(_p(marks), ctypes.c_int64(marks.size), ctypes.c_float(l_hit), ctypes.c_float(l_miss),
                                ctypes.c_float(l_min), ctypes.c_float(l_max), _p(log_odds), _p(observed))


def log_odds_constants(prob_hit=0.7, prob_miss=0.4, clamp=(0.12, 0.97)):
    """(l_hit, l_miss, l_min, l_max): log(p / (1 - p)) in float64, rounded to float32 once."""
    return tuple(np.float32(np.log(p / (1.0 - p))) for p in (prob_hit, prob_miss, clamp[0], clamp[1]))


# ---------------------------------------------------------------- the ray sets the tests share
def world(lat, s):
    """World coordinates (float32) of lattice coordinates s (..., 3): fmin + s * fres in float64, rounded once."""
    fmin = np.array(list(lat.fmin), np.float64)
    fres = np.array(list(lat.fres), np.float64)
    return (fmin + np.asarray(s, np.float64) * fres).astype(np.float32)


def generic_rays(lat, count, seed):
    """Seeded random rays in lattice coordinates: origins up to three cells outside the grid, endpoints inside its range."""
    rng = np.random.default_rng(seed)
    n = np.array(lat.dims, np.float64)
    o = rng.uniform(-3.5, n + 2.5, size=(count, 3))
    e = rng.uniform(0.05, n - 1.05, size=(count, 3))
    return world(lat, o), world(lat, e)


def axis_rays(lat, axis):
    """(origins (16, 3), endpoints (16, 3)) float32: rays that run the whole length of `axis` -- the four diagonals between the
    centres of opposite corner voxels, a ray through voxel centres from end to end and one from outside to outside, one on a
    cell face and one on a cell edge (half-integer lattice coordinates on the other axes), each in both directions."""
    n = np.array(lat.dims, np.float64)
    p, q = (axis + 1) % 3, (axis + 2) % 3
    pairs = []
    for sp in (0, 1):
        for sq in (0, 1):  # corner to opposite corner
            a, b = np.zeros(3), n - 1
            a[p], b[p] = (b[p], 0.0) if sp else (0.0, b[p])
            a[q], b[q] = (b[q], 0.0) if sq else (0.0, b[q])
            pairs.append((a, b))
    for ends, off_p, off_q in (((0.0, n[axis] - 1), 0.0, 1.0), ((-3.0, n[axis] + 2), 1.0, 0.0),  # through voxel centres
                               ((-1.25, n[axis] + 0.25), 0.5, 0.0), ((0.0, n[axis] - 1), 0.5, 0.5)):  # on a face, on an edge
        a, b = np.zeros(3), np.zeros(3)
        a[axis], b[axis] = ends
        a[p] = b[p] = off_p
        a[q] = b[q] = off_q
        pairs.append((a, b))
    so = np.array([a for a, b in pairs] + [b for a, b in pairs])
    se = np.array([b for a, b in pairs] + [a for a, b in pairs])
    return world(lat, so), world(lat, se)


def mixed_rays(lat, R, seed):
    """(origins (R, 3), endpoints (R, 3)) float32: every kind of ray the contract has a statement for, in a seeded shuffle.
    Origins inside and outside the grid, endpoints outside it, rays with one or two zero components, rays through cell corners
    and along cell faces (half-integer lattice coordinates), zero-length rays, non-finite rays."""
    rng = np.random.default_rng(seed)
    n = np.array(lat.dims, np.float64)
    so = rng.uniform(-3.5, n + 2.5, size=(R, 3))
    se = rng.uniform(-3.5, n + 2.5, size=(R, 3))
    kind = rng.integers(0, 10, size=R)
    inside = rng.uniform(-0.45, n - 0.55, size=(R, 3))
    so[kind == 0] = inside[kind == 0]                       # origin inside
    se[kind == 1] = inside[kind == 1]                       # endpoint inside, origin anywhere
    both = kind == 2                                        # both inside
    so[both], se[both] = inside[both], rng.uniform(-0.45, n - 0.55, size=(int(both.sum()), 3))
    for i in np.flatnonzero(kind == 3):                     # one zero component
        k = rng.integers(0, 3)
        so[i] = inside[i]
        se[i, k] = so[i, k]
    for i in np.flatnonzero(kind == 4):                     # two zero components: axis-parallel
        k = rng.integers(0, 3)
        so[i] = inside[i]
        keep = se[i, k]
        se[i] = so[i]
        se[i, k] = keep
    half = (kind == 5) | (kind == 6)                        # corners and faces: half-integer coordinates
    so[half] = np.floor(so[half]) + 0.5
    se[half] = np.floor(se[half]) + 0.5
    face = kind == 6                                        # along a face: one coordinate stays on a half-integer
    se[face, 0] = so[face, 0]
    so[kind == 7] = np.rint(inside[kind == 7])              # through voxel centres
    se[kind == 7] = np.rint(se[kind == 7])
    point_inside = (kind == 8) & (rng.random(R) < 0.7)      # zero length, inside or outside
    so[point_inside] = inside[point_inside]
    se[kind == 8] = so[kind == 8]
    o, e = world(lat, so), world(lat, se)
    bad = np.flatnonzero(kind == 9)                         # non-finite, in either end
    values = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j, i in enumerate(bad):
        (o if j % 2 else e)[i, rng.integers(0, 3)] = values[j % 3]
    return o, e
