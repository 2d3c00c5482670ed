"""Restatement of the surface-extraction contract (include/pvamd.h "Surface extraction") for its tests -- TEST INFRASTRUCTURE:
surface_ref.c compiled on the fly, and what the CPU and GPU tests share on top of the fields of tests/redistance_ref.py."""
import ctypes
from typing import NamedTuple

import numpy as np

from tests import c_ref
from tests.redistance_ref import bits  # noqa: F401  (re-exported for the tests)


class Mesh(NamedTuple):
    vertices: np.ndarray  # (rows, 3) float32: rows = min(count, capacity)
    normals: np.ndarray   # (rows, 3) float32, None when not asked for
    faces: np.ndarray     # (rows, 3) int32
    counts: tuple         # (vertices, triangles) of the whole mesh, whatever the capacities
    ids: np.ndarray       # (nx, ny, nz) int32: the vertex id of the cell whose lowest corner is the voxel, -1 without one


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _call(records, valid, fmin, fres, level, max_vertices, max_faces, want_normals):
    nx, ny, nz = records.shape[:3]
    vertices = np.zeros((max_vertices, 3), np.float32)
    normals = np.zeros((max_vertices, 3), np.float32) if want_normals else None
    faces = np.zeros((max_faces, 3), np.int32)
    ids = np.empty((nx, ny, nz), np.int32)
    counts = np.zeros((2,), np.int64)
    c_ref.load("surface_ref").surface_ref(_p(records), _p(valid), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), _p(fmin),
                                          _p(fres), ctypes.c_float(level), ctypes.c_int64(max_vertices), ctypes.c_int64(max_faces),
                                          _p(vertices), _p(normals), _p(faces), _p(ids), _p(counts))
    return vertices, normals, faces, ids, (int(counts[0]), int(counts[1]))


def extract(records, valid=None, fmin=(0.0, 0.0, 0.0), fres=(1.0, 1.0, 1.0), level=0.0, normals=True, max_vertices=None,
            max_faces=None):
    """Mesh of (nx, ny, nz, 4) float32 records over the lattice (fmin, fres); valid: (nx, ny, nz) uint8 or None.  Capacities of None:
    the counts, found by a first call with capacities of zero."""
    assert records.dtype == np.float32 and records.flags.c_contiguous and records.ndim == 4 and records.shape[3] == 4
    if valid is not None:
        valid = np.ascontiguousarray(valid, np.uint8)
        assert valid.shape == records.shape[:3]
    fmin, fres = np.asarray(fmin, np.float32), np.asarray(fres, np.float32)
    if max_vertices is None or max_faces is None:
        total = _call(records, valid, fmin, fres, level, 0, 0, False)[4]
        max_vertices = total[0] if max_vertices is None else max_vertices
        max_faces = total[1] if max_faces is None else max_faces
    vertices, nrm, faces, ids, counts = _call(records, valid, fmin, fres, level, max_vertices, max_faces, normals)
    return Mesh(vertices[:counts[0]], None if nrm is None else nrm[:counts[0]], faces[:counts[1]], counts, ids)


def families(mesh, shape):
    """((3,) quads per family, a (quads, 3), k (quads,)) of a complete mesh: a quad of family k at voxel a has C0 as the first and
    C2 = a as the third vertex of its first triangle."""
    cell_of = np.full((mesh.counts[0],), -1, np.int64)
    flat = np.flatnonzero(mesh.ids.reshape(-1) >= 0)
    cell_of[mesh.ids.reshape(-1)[flat]] = flat
    quads = mesh.faces[0::2]
    a = np.stack(np.unravel_index(cell_of[quads[:, 2]], shape), axis=1)
    c0 = np.stack(np.unravel_index(cell_of[quads[:, 0]], shape), axis=1)
    same = (a - c0) == 0  # C0 = a - e_p - e_q: the one axis along which they agree is k
    assert (same.sum(axis=1) == 1).all()
    k = same.argmax(axis=1)
    return np.bincount(k, minlength=3), a, k


def mask(shape, seed=3, fraction=0.05):
    """(valid (nx, ny, nz) uint8 with `fraction` of it zero, at least one voxel; bad (nx, ny, nz) int8: 0, or 1 / 2 / 3 where the
    sample is to be replaced by NaN / +inf / -inf, one voxel in 200), seeded."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    valid = np.ones(shape, np.uint8)
    valid.reshape(-1)[rng.choice(n, size=max(1, round(fraction * n)), replace=False)] = 0
    bad = np.zeros(shape, np.int8)
    where = rng.choice(n, size=n // 200, replace=False)
    bad.reshape(-1)[where] = rng.integers(1, 4, size=where.size)
    return valid, bad


def with_bad(records, bad):
    """A copy of the records with the samples `bad` marks replaced."""
    out = np.array(records)
    for code, value in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        out[..., 0][bad == code] = value
    return out
