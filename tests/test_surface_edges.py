"""Surface extraction without a GPU, on the inputs of tests/test_surface_edges_gpu.py: dense and irregular fields on lattices whose
arithmetic rounds and on thin shapes.  What that file compares the device with is the C restatement (tests/surface_ref.c); here
the restatement on those inputs is tied to things that are not it -- the numpy formulation of tests/test_surface.py, counts in
closed form, the box of every vertex's cell in float64 -- and the conditions the inputs are chosen for are shown to hold."""
import numpy as np
import pytest

from tests import redistance_ref
from tests import surface_ref as ref
from tests.test_surface import numpy_nets

bits = ref.bits
FIELDS = {"smooth": redistance_ref.smooth_field, "noise": ref.noise_field, "checker": ref.checker_field, "huge": ref.huge_field}
THIN = [(2, 9, 70), (9, 2, 70), (9, 70, 2), (2048, 2, 3), (2, 2048, 3), (3, 2, 2048), (3, 3, 2048)]


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("name", ["fine", "aniso"])
@pytest.mark.parametrize("field", ["noise", "checker"])
@pytest.mark.parametrize("shape", [(7, 5, 6), (2, 5, 6)])
def test_the_restatement_equals_the_numpy_formulation_on_dense_fields_and_rounding_lattices(shape, field, name, level):
    rec = FIELDS[field](shape)
    fmin, fres = ref.lattice(name)
    got = ref.extract(rec, None, fmin, fres, level)
    vertices, faces = numpy_nets(rec[..., 0], fmin, fres, level)
    assert got.counts == (len(vertices), len(faces)) and got.counts[0] >= 5 and got.counts[1] >= 4
    assert np.array_equal(bits(got.vertices), bits(vertices)) and np.array_equal(got.faces, faces)
    if field == "checker":
        assert got.counts == ref.checker_counts(shape)[0]


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("shape", THIN + [(2, 2, 2), (3, 3, 3), (7, 5, 6), (9, 8, 70), (17, 16, 64)])
def test_a_checker_field_has_the_counts_of_the_closed_form(shape, level):
    mesh = ref.extract(ref.checker_field(shape), level=level)
    counts, quads = ref.checker_counts(shape)
    assert mesh.counts == counts
    assert (mesh.ids[:-1, :-1, :-1] >= 0).all()  # every cell
    if counts[1]:
        assert np.array_equal(ref.families(mesh, shape)[0], quads)
    assert {(9, 8, 70): (3864, 18988), (17, 16, 64): (15120, 82136), (3, 3, 2048): (8188, 20462)}.get(shape, counts) == counts
    if 2 in shape and shape != (2, 2, 2):  # an axis of two voxels: quads only round the edges along it
        assert [q > 0 for q in quads] == [s == 2 for s in shape]


def inside_its_cell(mesh, shape, fmin, fres):
    """Every vertex lies in the closed box of its own cell, the cell being that of mesh.ids.

    In float32 with no margin at all: S_j / m is in [0, 1] (every f is, rounding is monotone and 0, 1 and the partial sums' bounds
    are floats), so p_j is in [c_j, c_j + 1], and fmin + p * fres rounds monotonically: the vertex lies between the float32
    centres of voxel c_j and c_j + 1, which by statement 4. are fmin + (float)c * fres in the same two roundings.

    In float64, where the box is [fmin + c * fres, fmin + (c + 1) * fres] without rounding (a 24-bit by 11-bit product, a sum
    whose error is 2^-53 relative): the float32 vertex took two roundings, each at most half an ulp of its result, 2^-24 relative.
    The product is at most span_j = (n_j - 1) * fres_j, the sum at most M_j = max(|fmin_j|, |fmin_j + span_j|).  The margin is
    2^-24 * (span_j + M_j), about one ulp of the coordinate, times (1 + 2^-10) for the roundings of the bound itself."""
    cells = ref.cells_of(mesh)
    assert (cells >= 0).all() and (cells <= np.array(shape) - 2).all()
    f32 = np.float32
    low32, high32 = fmin + cells.astype(f32) * fres, fmin + (cells + 1).astype(f32) * fres
    assert low32.dtype == np.float32 and ((low32 <= mesh.vertices) & (mesh.vertices <= high32)).all()
    fmin64, fres64 = fmin.astype(np.float64), fres.astype(np.float64)
    span = (np.array(shape) - 1) * fres64
    margin = 2.0 ** -24 * (span + np.maximum(np.abs(fmin64), np.abs(fmin64 + span))) * (1 + 2.0 ** -10)
    assert (margin < 1e-4 * fres64).all()  # a margin that tells a cell from its neighbour
    low, high = fmin64 + cells * fres64, fmin64 + (cells + 1) * fres64
    P = mesh.vertices.astype(np.float64)
    assert ((low - margin <= P) & (P <= high + margin)).all(), (np.max(low - P, axis=0), np.max(P - high, axis=0), margin)
    return cells


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("field", ["smooth", "noise", "checker", "huge"])
def test_on_the_anisotropic_lattice_every_vertex_lies_in_its_cell_and_every_face_names_vertices(field, level):
    shape = (19, 13, 37)
    rec = FIELDS[field](shape)
    fmin, fres = ref.lattice("aniso")
    mesh = ref.extract(rec, None, fmin, fres, level)
    assert mesh.counts[0] > 1000 and mesh.counts[1] > 1000
    cells = inside_its_cell(mesh, shape, fmin, fres)
    assert len(np.unique(np.ravel_multi_index(tuple(cells.T), shape))) == mesh.counts[0]  # a vertex per cell, a cell per vertex
    assert mesh.faces.min() >= 0 and mesh.faces.max() < mesh.counts[0]
    assert np.isfinite(mesh.vertices).all() and np.isfinite(mesh.normals).all()
    # the coordinates really take the per-axis resolution: the mesh spans its lattice on every axis
    extent = mesh.vertices.max(axis=0).astype(np.float64) - mesh.vertices.min(axis=0)
    assert (extent > 0.9 * (np.array(shape) - 1) * fres).all() and (extent <= (np.array(shape) - 1) * fres * (1 + 1e-6)).all()


@pytest.mark.parametrize("name, shape, axes", [("fine", (19, 13, 37), (0, 1, 2)), ("aniso", (19, 13, 37), (0, 1, 2)),
                                               ("limit", (2048, 2, 3), (0,)), ("limit", (2, 2048, 3), (1,)),
                                               ("limit", (3, 2, 2048), (2,)), ("limit", (3, 3, 2048), (2,))])
def test_on_these_lattices_a_fused_world_coordinate_would_show(name, shape, axes):
    """The condition the lattices are chosen for; on the dyadic lattice of tests/test_surface_gpu.py it does not hold."""
    rec = ref.noise_field(shape)
    differ = ref.fused_differ(rec, None, *ref.lattice(name))
    print(name, shape, differ, "of", ref.extract(rec, normals=False).counts[0])
    assert (differ[list(axes)] > 100).all()
    assert not ref.fused_differ(ref.noise_field((19, 13, 37)), None, (-1.25, 0.5, 3.0), (0.5, 0.5, 0.5)).any()


def test_the_huge_field_overflows_in_both_ways_and_the_restatement_stays_finite():
    shape = (9, 8, 70)
    rec = ref.huge_field(shape)
    V = rec[..., 0]
    assert np.isfinite(V).all() and 150 < (np.abs(V) > 1e38).sum() < 400 and (V == ref.FLT_MAX).any() and (V == -ref.FLT_MAX).any()
    assert np.array_equal(V < 0, ref.noise_field(shape)[..., 0] < 0)  # the signs are the noise field's
    whole = ref.extract(ref.noise_field(shape))
    for level in (0.0, 2.0e38, -2.0e38):
        edges, samples = ref.overflows(rec, level)
        mesh = ref.extract(rec, level=level)
        print(level, "W_a - W_b infinite on", edges, "crossings; W infinite at", samples, "finite samples;", mesh.counts)
        # about 14,000 edges, both ends huge on one in 400 and of opposite sign on half of those: 17 expected; 5 % of 5040 samples
        # are huge, and the half of them whose sign is not the level's overflows against 2e38: 126 expected
        assert (samples == 0 and edges >= 8) if level == 0.0 else samples > 50
        assert np.isfinite(mesh.vertices).all() and np.isfinite(mesh.normals).all() and mesh.counts[0] > 100 and mesh.counts[1] > 100
        if level == 0.0:  # usable and negative as in the noise field: the same cells and quads, other vertices
            assert mesh.counts == whole.counts and np.array_equal(mesh.ids, whole.ids) and np.array_equal(mesh.faces, whole.faces)
            assert not np.array_equal(bits(mesh.vertices), bits(whole.vertices))
        else:  # what deciding on V instead of W would mesh: the overflowed samples as if they were usable
            clipped = rec.copy()
            clipped[..., 0] = np.clip(V, -1e38, 1e38)
            assert ref.extract(clipped, level=level).counts != mesh.counts


def test_the_valid_bytes_hold_every_value_and_mean_what_their_truth_value_means():
    shape = (9, 8, 70)
    valid = ref.valid_bytes(shape)
    values, counts = np.unique(valid, return_counts=True)
    assert tuple(values) == ref.VALID_BYTES and counts.min() > 100 and 150 < counts[0] < 400
    rec = ref.huge_field(shape)
    as_given, as_bool = ref.extract(rec, valid), ref.extract(rec, (valid != 0).astype(np.uint8))
    assert as_given.counts == as_bool.counts and as_given.counts[0] > 1000 and as_given.counts[1] > 1000
    for a, b in zip(as_given[:3], as_bool[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert ref.extract(rec, (valid == 1).astype(np.uint8)).counts[0] < as_given.counts[0] // 4  # and not what == 1 means
