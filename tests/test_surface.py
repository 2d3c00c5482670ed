"""Surface extraction without a GPU: the contract's statements (include/pvamd.h "Surface extraction") on their C restatement
(tests/surface_ref.c) -- against an independent numpy formulation, on the analytic ball, rule by rule on small lattices and on
a fused TSDF ball -- and the argument errors of the Python layer and the entry points."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import surface as surface_module
from tests import redistance_ref
from tests import surface_ref as ref
from tests import tsdf_ref

bits = ref.bits


# ---------------------------------------------------------------- an independent formulation: shifted slices in float32
def numpy_nets(V, fmin, fres, level=0.0):
    """(vertices (Nv, 3) float32, faces (Nf, 3) int32) of a finite float32 field by whole-array operations, each rounded to
    float32 on its own.  Shares no code with the restatement."""
    f32 = np.float32
    W = V.astype(f32) - f32(level)
    n = W.shape
    cells = tuple(s - 1 for s in n)
    corner = lambda off: tuple(slice(off[j], n[j] - 1 + off[j]) for j in range(3))  # noqa: E731
    negatives = sum((W[corner((dx, dy, dz))] < 0).astype(int) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    active = (negatives > 0) & (negatives < 8)
    S, m = np.zeros(cells + (3,), f32), np.zeros(cells, int)
    for k in range(3):
        o0, o1 = [j for j in range(3) if j != k]
        for d0 in (0, 1):
            for d1 in (0, 1):
                low, high = [0, 0, 0], [0, 0, 0]
                low[o0] = high[o0] = d0
                low[o1] = high[o1] = d1
                high[k] = 1
                a, b = W[corner(low)], W[corner(high)]
                cross = (a < 0) != (b < 0)
                with np.errstate(all="ignore"):
                    f = a / (a - b)
                offset = np.zeros(cells + (3,), f32)
                offset[..., k], offset[..., o0], offset[..., o1] = f, f32(d0), f32(d1)
                S = np.where(cross[..., None], S + offset, S)
                m += cross
    ids = np.full(cells, -1, np.int64)
    ids[active] = np.arange(active.sum())
    p = np.argwhere(active).astype(f32) + S[active] / m[active].astype(f32)[:, None]
    vertices = np.asarray(fmin, f32) + p * np.asarray(fres, f32)
    keys, quads = [], []
    for k in range(3):
        p_, q_ = (k + 1) % 3, (k + 2) % 3
        lo = [0, 0, 0]
        lo[p_] = lo[q_] = 1
        at = tuple(slice(lo[j], n[j] - 1) for j in range(3))  # a: a cell of its own, with cells below it along p and q

        def shifted(dp, dq):
            off = [0, 0, 0]
            off[p_], off[q_] = dp, dq
            return ids[tuple(slice(lo[j] - off[j], n[j] - 1 - off[j]) for j in range(3))]

        c0, c1, c2, c3 = shifted(1, 1), shifted(0, 1), shifted(0, 0), shifted(1, 0)
        wa = W[at]
        up = [0, 0, 0]
        up[k] = 1
        wb = W[tuple(slice(lo[j] + up[j], n[j] - 1 + up[j]) for j in range(3))]
        emit = ((wa < 0) != (wb < 0)) & (c0 >= 0) & (c1 >= 0) & (c2 >= 0) & (c3 >= 0)
        a = np.argwhere(emit) + np.array(lo)
        inside = (wa < 0)[emit]
        v0, v2 = c0[emit], c2[emit]
        v1, v3 = np.where(inside, c1[emit], c3[emit]), np.where(inside, c3[emit], c1[emit])
        keys.append(np.ravel_multi_index(tuple(a.T), n) * 3 + k)
        quads.append(np.stack((v0, v1, v2, v0, v2, v3), axis=1))
    order = np.argsort(np.concatenate(keys), kind="stable")
    faces = np.concatenate(quads)[order].reshape(-1, 3).astype(np.int32)
    return vertices, faces


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 3, 3), (7, 5, 6)])
def test_the_restatement_equals_an_independent_numpy_formulation(shape, level):
    rec = redistance_ref.smooth_field(shape)
    fmin, fres = (-0.3, 0.1, 2.0), (0.02, 0.05, 0.125)
    got = ref.extract(rec, None, fmin, fres, level)
    vertices, faces = numpy_nets(rec[..., 0], fmin, fres, level)
    assert got.counts == (len(vertices), len(faces))
    assert np.array_equal(bits(got.vertices), bits(vertices)) and np.array_equal(got.faces, faces)
    assert got.counts[0] >= 1 and (shape == (2, 2, 2)) == (got.counts[1] == 0)  # one cell: a vertex and nothing to join it to


def test_signed_zeros_and_denormals_follow_the_comparison_and_the_division_as_stated():
    rec, tiny = redistance_ref.tiny_field((19, 13, 37))
    got = ref.extract(rec)
    vertices, faces = numpy_nets(rec[..., 0], (0, 0, 0), (1, 1, 1))
    assert np.array_equal(bits(got.vertices), bits(vertices)) and np.array_equal(got.faces, faces)
    touched = np.zeros(tiny.shape, bool)  # cells with a tiny sample at a corner
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                touched[:-1, :-1, :-1] |= tiny[dx:tiny.shape[0] - 1 + dx, dy:tiny.shape[1] - 1 + dy, dz:tiny.shape[2] - 1 + dz]
    assert (touched & (got.ids >= 0)).sum() > 100
    # -0.0 is not negative: among positive samples it makes no surface; a negative denormal does
    values = np.ones((2, 2, 2), np.float32)
    values[1, 0, 1] = -0.0
    assert ref.extract(redistance_ref.as_records(values)).counts == (0, 0)
    values[1, 0, 1] = -3e-39
    mesh = ref.extract(redistance_ref.as_records(values))
    assert mesh.counts == (1, 0)
    # the edges along x and z end in the corner, f = 1 / (1 + 3e-39) = 1; the one along y starts there, f = 3e-39 / (3e-39 + 1)
    f = np.float32(-3e-39) / (np.float32(-3e-39) - np.float32(1.0))
    assert 0 < f / np.float32(3) < 1.2e-38 and np.array_equal(mesh.vertices[0], np.array([1.0, f / np.float32(3), 1.0], np.float32))


# ---------------------------------------------------------------- the analytic ball
R, H_ = redistance_ref.BALL_RADIUS, redistance_ref.BALL_RES
BALL_LATTICE = dict(fmin=(-0.5, -0.5, -0.5), fres=(H_, H_, H_))


@functools.lru_cache(maxsize=None)
def ball():
    """(mesh of the restatement, world vertices float64): the 51^3 ball, values clipped to +/-0.06 in float32, level 0, with the
    analytic radial gradients."""
    values, _ = redistance_ref.ball_values()
    c = np.linspace(-0.5, 0.5, 51)
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1)
    radial = centres / np.maximum(np.linalg.norm(centres, axis=-1, keepdims=True), 1e-12)
    mesh = ref.extract(redistance_ref.as_records(values, radial), **BALL_LATTICE)
    return mesh, mesh.vertices.astype(np.float64)


def test_the_ball_is_closed_oriented_and_of_genus_zero():
    mesh, _ = ball()
    assert mesh.counts == (4184, 8364) == (len(mesh.vertices), len(mesh.faces))  # the float64 prototype's counts: float32 keeps them
    F = mesh.faces.astype(np.int64)
    directed = np.concatenate((F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]))
    assert len(np.unique(directed, axis=0)) == len(directed)  # every directed edge once
    undirected, uses = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    assert (uses == 2).all() and len(undirected) == 12546
    assert len(mesh.vertices) - len(undirected) + len(F) == 2
    assert len(np.unique(F)) == len(mesh.vertices)  # away from the border every vertex is named


def test_the_ball_faces_point_outward_and_enclose_its_volume():
    mesh, P = ball()
    t = P[mesh.faces]
    normal, centroid = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), t.mean(axis=1)
    assert ((normal * centroid).sum(axis=1) > 0).all()
    volume = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6
    true = 4 / 3 * math.pi * R ** 3
    print(f"volume {volume:.6f} against {true:.6f}: {100 * (volume / true - 1):+.2f} %")
    assert abs(volume / true - 1) < 0.01  # the prototype: 0.51 % low


def test_the_ball_vertices_lie_within_the_sagitta_of_the_sphere():
    """In voxels.  Inside: the sagitta of a cell's diagonal, 3 h^2 / (8 r) = 0.025, plus the error of linear interpolation
    h^2 / (8 r) = 0.0083.  Outside: the interpolation error alone.  The prototype measured -0.0234 to 0.0000."""
    _, P = ball()
    error = (np.linalg.norm(P, axis=1) - R) / H_
    print(f"vertex error in voxels: {error.min():+.4f} to {error.max():+.4f}, mean |e| {np.abs(error).mean():.4f}")
    assert -0.035 <= error.min() and error.max() <= 0.01


def test_the_ball_normals_have_unit_length_and_are_radial():
    """A vertex normal is the normalised sum of gradients interpolated along the cell's edges, each a convex combination of unit
    radial vectors at two corners.  Every corner is within the cell's diagonal d = sqrt(3) h of the vertex and at least
    rho = r - 2 h from the centre, and radial directions at two such points differ by at most 2 asin(d / (2 rho)) = 7.7 degrees:
    so does any convex combination of them from the radial direction at the vertex."""
    mesh, P = ball()
    length = np.linalg.norm(mesh.normals.astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 1e-6
    cosine = (mesh.normals * P).sum(axis=1) / np.linalg.norm(P, axis=1)
    bound = 2 * math.asin(math.sqrt(3) * H_ / (2 * (R - 2 * H_)))
    worst = math.degrees(np.arccos(np.clip(cosine, -1, 1)).max())
    print(f"worst angle to the radial direction {worst:.3f} degrees, bound {math.degrees(bound):.2f}")
    assert worst <= math.degrees(bound) < 8.0


# ---------------------------------------------------------------- the rules, one at a time
SMALL = (5, 4, 6)


def in_cells(mesh):
    """The faces with every vertex id replaced by the flat index of its cell: comparable between meshes with different ids."""
    cell_of = np.full((mesh.counts[0],), -1, np.int64)
    flat = np.flatnonzero(mesh.ids.reshape(-1) >= 0)
    cell_of[mesh.ids.reshape(-1)[flat]] = flat
    return cell_of[mesh.faces]


@pytest.mark.parametrize("how", ["nan", "inf", "-inf", "valid"])
def test_a_cell_with_an_unusable_corner_emits_nothing_and_its_neighbours_keep_their_bits(how):
    rec = redistance_ref.smooth_field(SMALL)
    whole = ref.extract(rec)
    at = (2, 1, 3)
    valid = None
    if how == "valid":
        valid = np.ones(SMALL, np.uint8)
        valid[at] = 0
    else:
        rec = rec.copy()
        rec[at][0] = float(how)
    holed = ref.extract(rec, valid)
    round_it = np.zeros(SMALL, bool)
    round_it[at[0] - 1:at[0] + 1, at[1] - 1:at[1] + 1, at[2] - 1:at[2] + 1] = True  # the eight cells with `at` as a corner
    assert (whole.ids[round_it] >= 0).sum() >= 4 and (holed.ids[round_it] == -1).all()
    assert np.array_equal(holed.ids[~round_it] >= 0, whole.ids[~round_it] >= 0)
    keep = (whole.ids >= 0) & ~round_it
    assert np.array_equal(bits(holed.vertices[holed.ids[keep]]), bits(whole.vertices[whole.ids[keep]]))
    assert np.array_equal(bits(holed.normals[holed.ids[keep]]), bits(whole.normals[whole.ids[keep]]))
    before = in_cells(whole).reshape(-1, 6)
    gone = round_it.reshape(-1)[before].any(axis=1)
    assert gone.sum() >= 3 and np.array_equal(in_cells(holed).reshape(-1, 6), before[~gone])  # the quads round it vanish, in order


def test_a_level_is_the_zero_level_of_the_shifted_field():
    rng = np.random.default_rng(4)
    values = rng.integers(-9, 10, size=(6, 5, 7)).astype(np.float32) / 4 + np.float32(0.125)  # dyadic: values - 0.25 is exact
    gradients = rng.standard_normal((6, 5, 7, 3))
    at_level = ref.extract(redistance_ref.as_records(values, gradients), level=0.25)
    shifted = ref.extract(redistance_ref.as_records(values - np.float32(0.25), gradients))
    assert at_level.counts == shifted.counts and at_level.counts[1] > 50
    for a, b in zip(at_level[:3], shifted[:3]):
        assert np.array_equal(bits(a), bits(b))


def test_the_orientation_flips_with_the_sign_of_the_field():
    rec = redistance_ref.smooth_field((7, 5, 6))
    assert (rec[..., 0] != 0).all()
    flipped = rec.copy()
    flipped[..., 0] = -flipped[..., 0]
    one, other = ref.extract(rec), ref.extract(flipped)
    assert np.array_equal(bits(one.vertices), bits(other.vertices)) and one.counts == other.counts and one.counts[1] > 50
    quads = one.faces.reshape(-1, 6)  # (v0, v1, v2, v0, v2, v3)
    assert np.array_equal(other.faces.reshape(-1, 6), quads[:, [0, 5, 2, 0, 2, 1]])


def test_quads_come_in_the_order_of_their_edges_and_every_edge_is_a_crossing_of_redistancing():
    shape = (7, 5, 6)
    rec = redistance_ref.smooth_field(shape)
    mesh = ref.extract(rec)
    per_family, a, k = ref.families(mesh, shape)
    assert (per_family > 5).all()
    keys = np.ravel_multi_index(tuple(a.T), shape) * 3 + k
    assert (np.diff(keys) > 0).all()
    assert np.array_equal(mesh.faces[0::2, 0], mesh.faces[1::2, 0]) and np.array_equal(mesh.faces[0::2, 2], mesh.faces[1::2, 1])
    # "Redistancing" 2.: the cost of the edge a quad was emitted for, seen from its own lower voxel, is finite iff it is a crossing
    sites = np.full((int(np.prod(shape)),), -1, np.int32)
    lower = np.ravel_multi_index(tuple(a.T), shape)
    for family in range(3):  # one edge per voxel and call
        sites[:] = -1
        sites[lower[k == family]] = (lower[k == family] * 4 + family).astype(np.int32)
        costs = redistance_ref.site_costs(rec, sites)
        assert np.isfinite(costs[lower[k == family]]).all() and np.isinf(np.delete(costs, lower[k == family])).all()


# ---------------------------------------------------------------- a fused TSDF ball
TRUNC, INTRINSICS = 0.06, (150.0, 150.0, 79.5, 59.5)


@functools.lru_cache(maxsize=None)
def fused_ball():
    """(lattice, state, records) of the ball of tests/test_tsdf.py: six axis views from one metre, fused by the restatement."""
    lat = tsdf_ref.make_lattice((51, 51, 51), (-0.5, -0.5, -0.5), H_)
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, INTRINSICS, 120, 160, (0.0, 0.0, 0.0), R)
    state = np.zeros(lat.dims + (2,), np.float32)
    tsdf_ref.integrate(lat, state, depth, tsdf_ref.invert(poses), INTRINSICS, TRUNC)
    return lat, state, tsdf_ref.records(state, H_, TRUNC).reshape(lat.dims + (4,))


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
def test_a_fused_ball_meshes_within_its_own_crossing_error_and_never_next_to_unseen_space(min_weight):
    """A vertex is the mean of crossings on its cell's edges: it is no further outside the sphere than the worst of them, and
    inside by at most the sagitta bound of the analytic ball, 0.035 voxel, more."""
    lat, state, rec = fused_ball()
    valid = state[..., 1] > min_weight
    mesh = ref.extract(rec, valid.astype(np.uint8), [lat.fmin[k] for k in range(3)], [lat.fres[k] for k in range(3)])
    c = tsdf_ref.centres(lat).astype(np.float64)
    val = rec[..., 0].astype(np.float64)
    worst = 0.0
    for axis in range(3):  # the worst lattice-edge crossing of this state
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = valid[a] & valid[b] & ((val[a] < 0) != (val[b] < 0))
        s = val[a][cross] / (val[a][cross] - val[b][cross])
        p = c[a][cross] + s[:, None] * (c[b][cross] - c[a][cross])
        worst = max(worst, (np.abs(np.linalg.norm(p, axis=1) - R) / H_).max())
    error = np.abs(np.linalg.norm(mesh.vertices.astype(np.float64), axis=1) - R) / H_
    print(f"min_weight {min_weight}: {mesh.counts} vertices and triangles, vertex error {error.max():.4f}, crossings {worst:.4f} voxels")
    assert mesh.counts[0] > 500 and mesh.counts[1] > 500  # weight > 1: only where two views overlap
    assert error.max() <= worst + 0.035
    corners_seen = np.ones(tuple(s - 1 for s in valid.shape), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                corners_seen &= valid[dx:50 + dx, dy:50 + dy, dz:50 + dz]
    assert not (mesh.ids[:-1, :-1, :-1] >= 0)[~corners_seen].any() and (mesh.ids[-1] == -1).all()
    assert (~valid).sum() > 1000


# ---------------------------------------------------------------- the Python layer and the entry points
def test_the_entry_points_reach_the_binding_and_refuse_bad_arguments_without_a_gpu():
    assert _lib.ABI_VERSION == 16
    assert [len(_lib.SIGNATURES[name][1]) for name in ("pvamd_surface_scratch_bytes", "pvamd_surface_count", "pvamd_surface_emit")] \
        == [3, 7, 11]
    assert _lib.SIGNATURES["pvamd_surface_scratch_bytes"][0] is ctypes.c_int64
    assert pv.extract_surface is surface_module.extract_surface and pv.Surface is surface_module.Surface
    assert _lib.SURFACE_MIN_AXIS == surface_module.MIN_AXIS == 2 and _lib.SURFACE_MAX_VOXELS == surface_module.MAX_VOXELS == 2 ** 29
    lib = _lib.load()
    E_NULL, E_SHAPE, E_MODE = (_lib.H[f"PVAMD_E_{name}"] for name in ("NULL", "SHAPE", "MODE"))
    for shape in ((1, 2, 2), (2, 2, 2049), (1024, 1024, 513)):
        assert lib.pvamd_surface_scratch_bytes(*shape) == 0
    n = 51 ** 3
    assert lib.pvamd_surface_scratch_bytes(51, 51, 51) == 7 * n + 8 * -(-n // _lib.H["PVAMD_SURFACE_CHUNK"])
    assert lib.pvamd_surface_scratch_bytes(1024, 1024, 512) > 7 * 2 ** 29
    desc = surface_module.lattice_desc((3, 4, 5), 0.02, (-0.5, 0.25, 1.0))
    assert [desc.fmin[k] for k in range(3)] == [-0.5, 0.25, 1.0] and desc.fres[0] == np.float32(0.02) and desc.finalized == 1
    fake = ctypes.c_void_p(1 << 12)  # refused before it is read
    assert lib.pvamd_surface_count(None, fake, None, 0.0, fake, fake, None) == E_NULL
    for level in (math.nan, math.inf, -math.inf):
        assert lib.pvamd_surface_count(ctypes.byref(desc), None, None, level, fake, fake, None) == E_MODE
        assert lib.pvamd_surface_emit(ctypes.byref(desc), None, None, level, fake, 1, 1, fake, None, fake, None) == E_MODE
    assert lib.pvamd_surface_count(ctypes.byref(desc), None, None, 0.0, fake, fake, None) == E_NULL
    assert lib.pvamd_surface_emit(ctypes.byref(desc), fake, None, 0.0, fake, 1, 1, None, None, fake, None) == E_NULL
    assert lib.pvamd_surface_emit(ctypes.byref(desc), None, None, math.nan, fake, -1, 1, fake, None, fake, None) == E_SHAPE
    unfinalized = _lib.GridDesc()
    for k in range(3):
        unfinalized.shape[k] = 4
    assert lib.pvamd_surface_count(ctypes.byref(unfinalized), fake, None, 0.0, fake, fake, None) == E_MODE
    unfinalized.shape[1] = 1
    assert lib.pvamd_surface_count(ctypes.byref(unfinalized), None, None, math.nan, fake, fake, None) == E_SHAPE  # the order


GOOD = torch.zeros((4, 5, 6))


@pytest.mark.parametrize("error, kwargs", [
    (ValueError, dict(values=torch.zeros((4, 5)))), (ValueError, dict(values=torch.zeros((4, 5, 6, 1)))),
    (ValueError, dict(values=torch.zeros((1, 5, 6)))), (ValueError, dict(values=torch.zeros((2, 2, 2049), dtype=torch.int8))),
    (ValueError, dict(values=torch.zeros((1024, 1024, 513), device="meta"))),
    (ValueError, dict(level=math.nan)), (ValueError, dict(level=math.inf)), (TypeError, dict(level="0")),
    (ValueError, dict(resolution=0.0)), (ValueError, dict(resolution=-1.0)), (ValueError, dict(resolution=math.inf)),
    (ValueError, dict(resolution=math.nan)), (ValueError, dict(origin=(0.0, 0.0))), (ValueError, dict(origin=(0.0, math.nan, 0.0))),
    (ValueError, dict(gradients=torch.zeros((4, 5, 6)))), (ValueError, dict(gradients=torch.zeros((4, 5, 6, 4)))),
    (ValueError, dict(valid=torch.ones((4, 5)))), (ValueError, dict(valid=torch.ones((4, 5, 7), dtype=torch.bool))),
    (TypeError, dict(values=torch.zeros((4, 5, 6), dtype=torch.complex64))),
])
def test_argument_errors_of_extract_surface_need_no_gpu(error, kwargs, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    with pytest.raises(error):
        pv.extract_surface(**{**dict(values=GOOD), **kwargs})


@pytest.mark.parametrize("error, kwargs", [
    (TypeError, dict(normals=1)), (TypeError, dict(normals=None)), (ValueError, dict(level=math.nan)), (ValueError, dict(level=-math.inf)),
    (ValueError, dict(min_weight=math.nan)), (TypeError, dict(min_weight="1")),
])
def test_argument_errors_of_a_volume_s_extract_mesh_need_no_gpu(error, kwargs, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    volume = pv.TSDFVolume(0.25, [(-1.0, 1.0), (-1.0, 1.0), (0.0, 1.5)], truncation=0.75, device="cpu")
    with pytest.raises(error):
        volume.extract_mesh(**kwargs)
    with pytest.raises(_lib.PvamdError):
        volume.extract_mesh()  # a volume in host memory: no CPU fallback


def test_a_surface_becomes_a_trimesh_on_the_host():
    vertices = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    surface = pv.Surface(vertices, torch.tensor([[0, 1, 2]], dtype=torch.int32), None)
    mesh = surface.to_trimesh()
    assert isinstance(mesh, pv.mesh_io.TriMesh) and mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64
    assert np.array_equal(mesh.vertices, vertices.numpy()) and mesh.faces.tolist() == [[0, 1, 2]]
    empty = pv.Surface(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32), None).to_trimesh()
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
