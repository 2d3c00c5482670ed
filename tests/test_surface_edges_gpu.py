"""-m gpu: surface extraction (csrc/surface.hip) bit for bit against the C restatement (tests/surface_ref.c) where
tests/test_surface_gpu.py does not go: lattices whose arithmetic rounds (one of them with a resolution per axis), shapes with an
axis of two voxels and of PVAMD_LATTICE_MAX_AXIS, fields on which every cell is active or the actives are irregular, chunk counts
at the scan's turn, samples whose W overflows, valid bytes other than 0 and 1, and the two chains from a volume back to geometry
through a distance transform and through redistancing.  Every comparison is equality of bits or of integers.
tests/test_surface_edges.py ties the restatement on these inputs to things that are not it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import helpers as H
from tests import redistance_ref
from tests import surface_ref as ref
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

assert_same = ref.assert_same
CHUNK, SCAN_WIDTH = _lib.H["PVAMD_SURFACE_CHUNK"], _lib.H["PVAMD_SURFACE_SCAN_WIDTH"]
FIELDS = {"smooth": redistance_ref.smooth_field, "noise": ref.noise_field, "checker": ref.checker_field, "huge": ref.huge_field}
THIN = [(2, 9, 70), (9, 2, 70), (9, 70, 2), (2048, 2, 3), (2, 2048, 3), (3, 2, 2048), (3, 3, 2048)]


def raw(rec, valid, fmin, fres, level=0.0, normals=True):
    """pvamd_surface_count and pvamd_surface_emit on (nx, ny, nz, 4) float32 records over any lattice, `valid` handed over byte
    for byte: (Surface, the counts the device reported, the valid bytes as they are afterwards)."""
    shape = rec.shape[:3]
    n = shape[0] * shape[1] * shape[2]
    lib = _lib.load()
    desc = ref.lattice_desc(shape, fres, fmin)
    records = torch.from_numpy(np.array(rec)).cuda().reshape(n, 4)
    valid_dev = None if valid is None else torch.from_numpy(np.array(valid)).cuda().reshape(n)
    scratch = _lib.scratch_buffer(_lib.surface_scratch_bytes(*shape), records.device)
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    _lib.check(lib.pvamd_surface_count(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid_dev), level, _lib.ptr(scratch),
                                       _lib.ptr(counts), _lib.stream_ptr()), "pvamd_surface_count")
    nv, nf = counts.tolist()
    vertices = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    out_normals = torch.empty((nv, 3), dtype=torch.float32, device="cuda") if normals else None
    faces = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    _lib.check(lib.pvamd_surface_emit(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid_dev), level, _lib.ptr(scratch), nv, nf,
                                      _lib.ptr(vertices), _lib.ptr(out_normals), _lib.ptr(faces), _lib.stream_ptr()),
               "pvamd_surface_emit")
    torch.cuda.synchronize()
    return pv.Surface(vertices, faces, out_normals), (nv, nf), None if valid is None else valid_dev.cpu().numpy().reshape(shape)


def run(name, rec, valid=None, level=0.0, normals=True):
    """The device's mesh of the records on LATTICES[name]: pv.extract_surface where the lattice is isotropic, the raw entry
    points where it is not."""
    fres, fmin = ref.LATTICES[name]
    if len(set(fres)) > 1:
        return raw(rec, valid, fmin, fres, level, normals)[0]
    values, gradients = torch.from_numpy(np.array(rec[..., 0])), torch.from_numpy(np.array(rec[..., 1:]))
    return pv.extract_surface(values, resolution=fres[0], origin=fmin, level=level, gradients=gradients if normals else None,
                              valid=None if valid is None else torch.from_numpy(np.array(valid)))


def restated(name, rec, valid=None, level=0.0, normals=True):
    return ref.extract(rec, valid, *ref.lattice(name), level, normals)


# ---------------------------------------------------------------- lattices that round
@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("field", ["smooth", "noise", "checker"])
@pytest.mark.parametrize("name", ["fine", "aniso", "far"])
def test_bit_for_bit_where_the_world_coordinates_round(name, field, masked, level):
    shape = (19, 13, 37)
    rec, valid = FIELDS[field](shape), None
    if masked:
        valid, bad = ref.mask(shape)
        rec = ref.with_bad(rec, bad)
    want = restated(name, rec, valid, level)
    assert_same(run(name, rec, valid, level), want)
    assert want.counts[0] > 1000 and want.counts[1] > 1000 and (ref.families(want, shape)[0] > 100).all()
    if name != "far":  # kept for the magnitude of its coordinates; tests/test_surface_edges.py has the counts of the others
        assert (ref.fused_differ(rec, valid, *ref.lattice(name), level) > 50).all()
    else:
        assert (np.abs(want.vertices) > 490).all()
    if field == "checker" and not masked:
        assert want.counts == ref.checker_counts(shape)[0]


def test_without_gradients_on_the_anisotropic_lattice():
    rec = ref.noise_field((19, 13, 37))
    assert_same(run("aniso", rec, normals=False), restated("aniso", rec, normals=False))


# ---------------------------------------------------------------- thin lattices and the axis limit
def last_cell(shape):
    """The largest flat index that can carry a vertex, which is also the largest that can carry a quad (of the family along an
    axis of two voxels, of any family without one): the lowest corner of the last cell."""
    return int(np.ravel_multi_index(tuple(s - 2 for s in shape), shape))


def check_thin(want, shape, field):
    """Conditions on the restatement's mesh of a thin shape, not on the device: which families have quads, and that vertices and
    quads reach the last chunk that can hold any."""
    per_family, a, _ = ref.families(want, shape)
    if 2 in shape:
        assert [q > 0 for q in per_family] == [s == 2 for s in shape]  # only round the edges along the axis of two voxels
    else:
        assert (per_family > 0).all()
    top_vertex = int(np.flatnonzero(want.ids.reshape(-1) >= 0).max())
    top_quad = int(np.ravel_multi_index(tuple(a.T), shape).max())
    assert top_vertex // CHUNK == top_quad // CHUNK == last_cell(shape) // CHUNK
    n = shape[0] * shape[1] * shape[2]
    if shape[0] > 2 and shape[1] * shape[2] + shape[2] + 1 < CHUNK:  # a last cell less than a chunk from the end: the last chunk
        assert last_cell(shape) // CHUNK == (n - 1) // CHUNK
    if field == "checker":
        counts, quads = ref.checker_counts(shape)
        assert want.counts == counts and np.array_equal(per_family, quads) and top_vertex == top_quad == last_cell(shape)
    return per_family


@pytest.mark.parametrize("field", ["noise", "checker"])
@pytest.mark.parametrize("shape", THIN)
def test_bit_for_bit_on_thin_lattices_and_on_an_axis_of_2048_voxels(shape, field):
    """On (2048, 2, 3) an x plane is six voxels: a wave spans ten planes and a chunk forty-two, and the cells below a voxel along x
    and y belong to other lanes of its own wave."""
    assert max(shape) in (70, _lib.LATTICE_MAX_AXIS)
    rec = FIELDS[field](shape)
    want = restated("limit", rec)
    got = run("limit", rec)
    assert_same(got, want)
    per_family = check_thin(want, shape, field)
    print(shape, field, want.counts, per_family)
    assert {((2, 9, 70), "checker"): 476, ((2048, 2, 3), "checker"): 2046}.get((shape, field), per_family.max()) == per_family.max()
    assert want.counts[0] > 400 and want.counts[1] > 400
    axis = int(np.argmax(shape))
    if shape[axis] == _lib.LATTICE_MAX_AXIS:
        assert ref.fused_differ(rec, None, *ref.lattice("limit"))[axis] > 100
        coordinate = want.vertices[:, axis].astype(np.float64)
        assert coordinate.max() - coordinate.min() > 2045 * 0.02  # vertices at both ends of the long axis


# ---------------------------------------------------------------- full ballots
@pytest.mark.parametrize("shape, full_wave", [((17, 16, 64), 63), ((9, 8, 70), 64)])
def test_every_cell_active_the_counts_are_the_closed_form_on_the_device_too(shape, full_wave):
    """The one place where the counts rest on something other than the restatement.  On (17, 16, 64) a z line is exactly a wave,
    whose last lane never has a cell: 63 actives in every wave that has any.  On (9, 8, 70) a line is longer than a wave and
    some waves hold 64 active cells, each with three quads."""
    rec = ref.checker_field(shape)
    counts, quads = ref.checker_counts(shape)
    assert counts == {(17, 16, 64): (15120, 82136), (9, 8, 70): (3864, 18988)}[shape]
    want = restated("limit", rec)
    assert want.counts == counts and np.array_equal(ref.families(want, shape)[0], quads)
    got, device_counts, _ = raw(rec, None, *ref.lattice("limit"))
    assert device_counts == counts
    assert_same(got, want)
    assert_same(run("limit", rec), want)
    active = want.ids.reshape(-1) >= 0
    waves = np.add.reduceat(active, np.arange(0, active.size, 64))
    assert waves.max() == full_wave
    _, a, _ = ref.families(want, shape)
    quads_at = np.bincount(np.ravel_multi_index(tuple(a.T), shape), minlength=active.size)
    assert np.add.reduceat(quads_at, np.arange(0, active.size, 64)).max() >= 3 * 62  # a wave whose ballots are nearly full thrice
    assert np.add.reduceat(active, np.arange(0, active.size, CHUNK)).max() >= CHUNK - 8


# ---------------------------------------------------------------- the scan's turns
SCAN_SHAPES = {(64, 64, 64): SCAN_WIDTH, (41, 80, 80): SCAN_WIDTH + 1, (2018, 10, 13): SCAN_WIDTH + 1,
               (64, 64, 128): H.STREAM_GRID_ITEMS // CHUNK}


@pytest.mark.parametrize("shape", list(SCAN_SHAPES))
def test_chunk_counts_at_the_turn_of_the_scan(shape):
    """1024 chunks: the scan's loop ends after one full turn.  1025: the second turn holds one chunk sum.  On (41, 80, 80) that
    chunk lies in the last x plane and its sums are zero; on (2018, 10, 13), a plane of 130 voxels, it holds cells and quads of
    the last but one plane, so that the carry of the first turn is added to something.  (64, 64, 128): as many voxels as the
    capped streaming grid has lanes."""
    n = shape[0] * shape[1] * shape[2]
    chunks = -(-n // CHUNK)
    assert chunks == SCAN_SHAPES[shape] and (CHUNK, SCAN_WIDTH) == (256, 1024)
    assert n == H.STREAM_GRID_ITEMS or chunks in (SCAN_WIDTH, SCAN_WIDTH + 1)
    rec = redistance_ref.smooth_field(shape)
    want = restated("fine", rec)
    got, device_counts, _ = raw(rec, None, *ref.lattice("fine"))
    assert device_counts == want.counts and want.counts[0] > 10000
    assert_same(got, want)
    if shape == (2018, 10, 13):
        tail = want.ids.reshape(-1)[SCAN_WIDTH * CHUNK:]
        _, a, _ = ref.families(want, shape)
        assert (tail >= 0).sum() > 5 and (np.ravel_multi_index(tuple(a.T), shape) >= SCAN_WIDTH * CHUNK).sum() > 5


# ---------------------------------------------------------------- W, not V
@pytest.mark.parametrize("level", [0.0, 2.0e38, -2.0e38])
def test_usable_is_decided_on_w_and_an_overflowing_difference_gives_f_of_zero(level):
    shape = (9, 8, 70)
    rec = ref.huge_field(shape)
    edges, samples = ref.overflows(rec, level)
    assert (samples == 0 and edges >= 8) if level == 0.0 else samples > 50  # tests/test_surface_edges.py says why these numbers
    want = restated("limit", rec, level=level)
    assert np.isfinite(want.vertices).all() and np.isfinite(want.normals).all() and want.counts[0] > 100 and want.counts[1] > 100
    assert_same(run("limit", rec, level=level), want)


# ---------------------------------------------------------------- valid bytes
def test_any_nonzero_valid_byte_is_usable_and_the_bytes_are_never_written():
    """Through the raw entry points only: pv.extract_surface hands over (valid != 0)."""
    shape = (9, 8, 70)
    rec, valid = ref.huge_field(shape), ref.valid_bytes(shape)
    assert set(np.unique(valid)) == set(ref.VALID_BYTES)
    want = restated("limit", rec, valid)
    as_bool = restated("limit", rec, (valid != 0).astype(np.uint8))
    assert want.counts == as_bool.counts and want.counts[0] > 1000 and want.counts[1] > 1000
    got, device_counts, valid_after = raw(rec, valid, *ref.lattice("limit"))
    assert device_counts == want.counts
    assert_same(got, want)
    assert_same(got, as_bool)
    assert np.array_equal(valid_after, valid)


# ---------------------------------------------------------------- chains from a volume back to geometry
def restated_cache(cached, normals=True):
    """(the restatement's mesh of a cache's own records over its own descriptor, records, fmin, fres)."""
    desc = cached._grid_desc()
    shape = tuple(desc.shape)
    records = cached._packed.cpu().numpy().reshape(shape + (4,))
    fmin, fres = np.array([desc.fmin[k] for k in range(3)], np.float32), np.array([desc.fres[k] for k in range(3)], np.float32)
    return ref.extract(records, None, fmin, fres, normals=normals), records, fmin, fres


def test_an_occupancy_map_meshes_through_its_distance_transform():
    """OccupancyMap -> to_sdf -> extract_mesh: records of a signed distance transform, +/-(d - 0.5) with d the root of an integer
    and exact ties wherever the ball is symmetric.  One scan from a corner with an endpoint in every voxel of a ball: a hit takes
    precedence over any number of crossings, so exactly the ball is occupied."""
    N, res, radius = 33, 0.02, 10.3
    omap = pv.OccupancyMap(res, [(-0.32, 0.32)] * 3, device="cuda")
    assert omap.shape == (N, N, N)
    desc = omap._grid.voxels._grid_desc()
    fmin, fres = np.array([desc.fmin[k] for k in range(3)], np.float64), np.array([desc.fres[k] for k in range(3)], np.float64)
    index = np.stack(np.meshgrid(*(np.arange(N),) * 3, indexing="ij"), axis=-1)
    ball = np.linalg.norm(index - (N - 1) / 2, axis=-1) <= radius
    centres = fmin + index[ball] * fres
    omap.integrate(torch.tensor(fmin - 0.25 * fres), torch.from_numpy(centres))
    occupied = omap.occupied().cpu().numpy()
    assert np.array_equal(occupied, ball) and 4000 < ball.sum() < 5000
    cached = omap.to_sdf("ball", signed=True)
    want, records, lattice_min, lattice_res = restated_cache(cached)
    assert np.array_equal(records[..., 0] < 0, ball)
    assert len(np.unique(np.abs(records[..., 0]))) < 400  # few distinct values among 35,937 samples: ties abound
    assert_same(cached.extract_mesh(), want)
    assert_same(cached.extract_mesh(normals=False), restated_cache(cached, normals=False)[0])
    assert want.counts[0] > 1000 and want.counts[1] > 2000
    # statement 3. from outside, in float64: the cell a vertex lies in has an occupied and a free corner
    P = (want.vertices.astype(np.float64) - lattice_min) / lattice_res
    cell = np.floor(P).astype(np.int64)
    assert np.abs(P - np.rint(P)).min() > 0.01  # no vertex so near a cell's face that float32 could move it across
    assert np.array_equal(cell, ref.cells_of(want)) and cell.min() >= 0 and cell.max() <= N - 2
    corners = np.stack([ball[cell[:, 0] + dx, cell[:, 1] + dy, cell[:, 2] + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)])
    assert (corners.any(axis=0) & ~corners.all(axis=0)).all()
    every, some = np.ones((N - 1,) * 3, bool), np.zeros((N - 1,) * 3, bool)  # and every such cell has a vertex
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                corner = ball[dx:N - 1 + dx, dy:N - 1 + dy, dz:N - 1 + dz]
                every &= corner
                some |= corner
    mixed = some & ~every
    assert mixed.sum() == want.counts[0] and np.array_equal(want.ids[:-1, :-1, :-1] >= 0, mixed)


R, BALL_RES, TRUNC, INTRINSICS = 0.3, 0.02, 0.06, (150.0, 150.0, 79.5, 59.5)


@functools.lru_cache(maxsize=1)
def fused_ball():
    """The 51^3 volume of tests/test_surface_gpu.py: a ball seen from six sides."""
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, INTRINSICS, 120, 160, (0.0, 0.0, 0.0), R)
    vol = pv.TSDFVolume(BALL_RES, [(-0.5, 0.5)] * 3, truncation=TRUNC, device="cuda")
    assert vol.shape == (51, 51, 51)
    vol.integrate(torch.from_numpy(depth), INTRINSICS, torch.from_numpy(poses))
    return vol


@pytest.mark.parametrize("unknown", ["free", "occupied"])
def test_a_volume_meshes_through_its_redistanced_records(unknown):
    """TSDFVolume -> to_sdf(far_field=True) -> extract_mesh: kept records inside the band, Euclidean ones beyond it.  With unknown
    space occupied the interior of the ball, which no camera saw, is negative and the far field runs through it."""
    cached = fused_ball().to_sdf("ball", unknown=unknown, far_field=True)
    want, records, _, _ = restated_cache(cached)
    assert (np.abs(records[..., 0]) > 2 * TRUNC).sum() > 10000 and np.isfinite(records).all()  # redistanced: beyond the truncation
    assert_same(cached.extract_mesh(), want)
    assert_same(cached.extract_mesh(normals=False), restated_cache(cached, normals=False)[0])
    assert want.counts[0] > 1000 and want.counts[1] > 1000
    print(unknown, want.counts)
