"""Restatement of the surface-extraction contract (include/pvamd.h "Surface extraction") for its tests -- TEST INFRASTRUCTURE:
surface_ref.c compiled on the fly, and what the CPU and GPU tests share on top of the fields of tests/redistance_ref.py."""
import ctypes
import functools
from typing import NamedTuple

import numpy as np

from tests import c_ref
from tests.redistance_ref import as_records, bits


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


def assert_same(got, want):
    """A Surface of device tensors (vertices, faces, normals) against a Mesh of the restatement: the counts and every bit."""
    assert (got.vertices.shape[0], got.faces.shape[0]) == want.counts
    for name, g, w in (("vertices", got.vertices, want.vertices), ("normals", got.normals, want.normals), ("faces", got.faces, want.faces)):
        if w is None:
            assert g is None, name
            continue
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (name, int((bits(g) != bits(w)).sum()))


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


# ---------------------------------------------------------------- lattices whose arithmetic rounds, and dense fields
# name: (resolution per axis, origin).  The first three are those of tests/test_volume_lattices_gpu.py; `aniso` has a resolution
# of its own on every axis, which only the raw entry points take.
LATTICES = {"fine": ((0.013, 0.013, 0.013), (3.37, -1.21, 0.113)), "far": ((0.02, 0.02, 0.02), (1000.37, -998.21, 500.113)),
            "limit": ((0.02, 0.02, 0.02), (3.37, -1.21, -20.0)), "aniso": ((0.013, 0.02, 0.031), (3.37, -1.21, 0.113))}
FLT_MAX = float(np.finfo(np.float32).max)
HUGE = (1.8e38, 3.0e38, FLT_MAX)  # finite; the difference of two of opposite sign overflows, and so does any of them - (-/+2e38)
VALID_BYTES = (0, 1, 2, 128, 255)


def _read_only(values, rng):
    rec = as_records(values, rng.standard_normal(values.shape + (3,)))
    rec.flags.writeable = False
    return rec


@functools.lru_cache(maxsize=None)
def checker_field(shape, seed=21):
    """(nx, ny, nz, 4) float32 records, read-only: sign (-1)^(x + y + z), magnitude uniform in [0.25, 1.75), noise for gradients.
    Every lattice edge carries a crossing and every cell is active (also at level 0.25: no positive sample goes below zero),
    so the counts are checker_counts(shape) and every ballot of the kernels has all the bits the lattice allows."""
    rng = np.random.default_rng(seed)
    x, y, z = np.indices(shape)
    return _read_only(np.where((x + y + z) % 2 == 0, 1.0, -1.0) * rng.uniform(0.25, 1.75, size=shape), rng)


def checker_counts(shape):
    """((vertices, triangles), (3,) quads per family) of a checker field by counting: a cell per (n - 1)^3, and a quad per edge
    along k whose lower voxel has a cell of its own and cells below it along the other two axes."""
    nx, ny, nz = shape
    quads = np.array([(nx - 1) * (ny - 2) * (nz - 2), (nx - 2) * (ny - 1) * (nz - 2), (nx - 2) * (ny - 2) * (nz - 1)])
    return ((nx - 1) * (ny - 1) * (nz - 1), 2 * int(quads.sum())), quads


@functools.lru_cache(maxsize=None)
def noise_field(shape, seed=22):
    """(nx, ny, nz, 4) float32 records, read-only: standard normal values, so that the active cells and the quads of a wave form
    irregular bit patterns with about half the bits set."""
    rng = np.random.default_rng(seed)
    return _read_only(rng.standard_normal(shape), rng)


@functools.lru_cache(maxsize=None)
def huge_field(shape, seed=23):
    """(nx, ny, nz, 4) float32 records, read-only: noise_field with about 5 % of the samples replaced by +/-HUGE, keeping their
    sign.  At level 0 every sample is usable and W_a - W_b overflows on some crossings (f = 0); at level +/-2e38 some finite V
    have an infinite W = V - level and are unusable."""
    rec = noise_field(shape).copy()
    rng = np.random.default_rng(seed)
    pick = rng.random(shape) < 0.05
    magnitude = rng.choice(np.array(HUGE, np.float32), size=shape)
    rec[..., 0][pick] = np.copysign(magnitude, rec[..., 0])[pick]
    rec.flags.writeable = False
    return rec


def overflows(records, level):
    """(crossing edges whose W_a - W_b is infinite, finite samples whose W is infinite) of records at a level, with valid = NULL."""
    with np.errstate(over="ignore", invalid="ignore"):
        V = records[..., 0]
        W = V - np.float32(level)
        usable = np.isfinite(W)
        edges = 0
        for axis in range(3):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(0, -1), slice(1, None)
            a, b = tuple(a), tuple(b)
            cross = usable[a] & usable[b] & ((W[a] < 0) != (W[b] < 0))
            edges += int((cross & np.isinf(W[a] - W[b])).sum())
    return edges, int((np.isfinite(V) & ~usable).sum())


@functools.lru_cache(maxsize=None)
def valid_bytes(shape, seed=24):
    """(nx, ny, nz) uint8, read-only: about 5 % zeros, the rest drawn evenly from the other VALID_BYTES.  Usable is != 0."""
    valid = np.random.default_rng(seed).choice(np.array(VALID_BYTES, np.uint8), size=shape, p=(0.05,) + (0.2375,) * 4)
    valid.flags.writeable = False
    return valid


def lattice(name):
    """(fmin, fres) of LATTICES[name] as (3,) float32: what a descriptor holds and the restatement is given."""
    fres, fmin = LATTICES[name]
    return np.asarray(fmin, np.float32), np.asarray(fres, np.float32)


def lattice_desc(shape, fres, fmin):
    """pytorch_volumetric_amd.surface.lattice_desc with a resolution per axis: a finalized pvamd_grid_t without storage whose
    float32 fields are fmin and fres."""
    from pytorch_volumetric_amd import _lib, voxel
    desc = _lib.GridDesc()
    for d in range(3):
        low, res = np.float32(fmin[d]), np.float32(fres[d])
        high = np.float32(low + np.float32(shape[d] - 1) * res)
        desc.fmin[d], desc.fmax[d], desc.fres[d] = float(low), float(high), float(res)
        desc.dmin[d], desc.dmax[d], desc.dres[d] = float(low), float(high), float(res)
        desc.shape[d] = shape[d]
    desc.index_f64 = 0
    desc.rule = voxel.INDEX_RULE
    desc.oob_mode = _lib.OOB_BOUNDING_BOX
    _lib.check(_lib.load().pvamd_grid_finalize(ctypes.byref(desc)), "pvamd_grid_finalize")
    return desc


def fused_differ(records, valid, fmin, fres, level=0.0):
    """(3,) how many vertex coordinates per axis a fused fmaf(p, fres, fmin) would change: p is the vertex on the unit lattice
    from the origin (0 + p * 1 is exact), and float64 holds p * fres exactly and the sum to 53 bits."""
    p = extract(records, valid, level=level, normals=False).vertices
    fmin, fres = np.asarray(fmin, np.float32), np.asarray(fres, np.float32)
    fused = (fmin.astype(np.float64) + p.astype(np.float64) * fres.astype(np.float64)).astype(np.float32)
    return (fused != fmin + p * fres).sum(axis=0)


def cells_of(mesh):
    """(vertices, 3) the cell of every vertex id, from mesh.ids."""
    flat = np.flatnonzero(mesh.ids.reshape(-1) >= 0)
    out = np.empty((mesh.counts[0], 3), np.int64)
    out[mesh.ids.reshape(-1)[flat]] = np.stack(np.unravel_index(flat, mesh.ids.shape), axis=1)
    return out
