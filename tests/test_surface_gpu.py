"""-m gpu: surface extraction on the device, bit for bit against the C restatement of the contract (tests/surface_ref.c), through
pv.extract_surface, the raw entry points, TSDFVolume.extract_mesh and CachedSDF.extract_mesh, and the mesh it hands to MeshSDF."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import surface as surface_module
from tests import helpers as H
from tests import redistance_ref
from tests import surface_ref as ref
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.5, (-1.25, 0.5, 3.0)
BIG = (96, 80, 72)
assert BIG[0] * BIG[1] * BIG[2] > H.STREAM_GRID_ITEMS
FIELDS = {"smooth": redistance_ref.smooth_field, "tie": redistance_ref.tie_field, "tiny": lambda shape: redistance_ref.tiny_field(shape)[0]}


def run(rec, valid=None, level=0.0, normals=True):
    """pv.extract_surface on (nx, ny, nz, 4) float32 records."""
    values, gradients = torch.from_numpy(np.array(rec[..., 0])), torch.from_numpy(np.array(rec[..., 1:]))
    got = pv.extract_surface(values, resolution=RES, origin=ORIGIN, level=level, gradients=gradients if normals else None,
                             valid=None if valid is None else torch.from_numpy(valid))
    assert isinstance(got, pv.Surface) and got.vertices.is_cuda and got.faces.is_cuda and not got.vertices.requires_grad
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert got.vertices.shape == (got.vertices.shape[0], 3) and got.faces.shape == (got.faces.shape[0], 3)
    assert (got.normals is None) == (not normals)
    return got


def restated(rec, valid=None, level=0.0, normals=True, **capacities):
    return ref.extract(rec, valid, ORIGIN, (RES, RES, RES), level, normals, **capacities)


assert_same = ref.assert_same  # shared with tests/test_surface_edges_gpu.py


# Which cases cannot have quads of all three families, by the contract itself (the restatement gives these counts): on (3, 3, 3) a
# family has two candidate edges, and the fields put crossings on few of them; on (5, 3, 131) the tie field's level set is a
# sphere about the centre so much wider than the lattice's x and y extent that only edges along z cross it.
def expect_all_families(shape, field):
    return shape not in ((2, 2, 2), (3, 3, 3)) and not (shape == (5, 3, 131) and field == "tie")


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("field", ["smooth", "tie", "tiny"])
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 3, 3), (5, 3, 131), (19, 13, 37)])  # (5, 3, 131): a z line spans waves, a wave lines
def test_vertices_normals_and_faces_bit_for_bit(shape, field, masked, level):
    rec, valid = FIELDS[field](shape), None
    if masked:
        valid, bad = ref.mask(shape)
        rec = ref.with_bad(rec, bad)
    want = restated(rec, valid, level)
    assert_same(run(rec, valid, level), want)
    per_family = ref.families(want, shape)[0] if want.counts[1] else np.zeros(3, int)
    print(shape, field, masked, level, want.counts, per_family)
    if expect_all_families(shape, field):
        assert (per_family > 0).all()
    if shape == (2, 2, 2):
        assert want.counts == ((0, 0) if masked else (1, 0))  # one cell: a vertex and no face; with a corner masked, nothing
    if shape == (3, 3, 3) and not masked and (field, level) != ("tie", 0.25):
        assert want.counts[1] > 0  # the smallest shape with a quad
    if masked and shape == (19, 13, 37):
        assert (valid == 0).sum() > 400 and np.isnan(rec[..., 0]).any() and np.isinf(rec[..., 0]).any()


def test_without_gradients_there_are_no_normals_and_the_same_vertices():
    rec = redistance_ref.smooth_field((19, 13, 37))
    assert_same(run(rec, normals=False), restated(rec, normals=False))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_field_without_a_crossing_gives_empty_tensors(sign):
    got = pv.extract_surface(torch.full((5, 3, 131), 2.0 * sign), gradients=torch.zeros((5, 3, 131, 3)))
    assert got.vertices.shape == (0, 3) and got.normals.shape == (0, 3) and got.faces.shape == (0, 3) and got.vertices.is_cuda


@functools.lru_cache(maxsize=1)
def big():
    """(records, the restatement's mesh) on the lattice past the streaming cap, worked out once."""
    rec = redistance_ref.smooth_field(BIG)
    return rec, restated(rec)


def test_past_the_streaming_cap_bit_for_bit():
    rec, want = big()
    assert_same(run(rec), want)
    n = BIG[0] * BIG[1] * BIG[2]
    tail = want.ids.reshape(-1)[H.STREAM_GRID_ITEMS:]
    assert (tail >= 0).sum() > 100  # vertices among the cells of the lanes' second turn
    _, a, _ = ref.families(want, BIG)
    assert (np.ravel_multi_index(tuple(a.T), BIG) >= H.STREAM_GRID_ITEMS).sum() > 100  # and quads
    chunks = -(-n // _lib.H["PVAMD_SURFACE_CHUNK"])
    assert _lib.surface_scratch_bytes(*BIG) == 7 * n + 8 * chunks
    assert chunks > _lib.H["PVAMD_SURFACE_SCAN_WIDTH"]  # the scan of the chunk sums takes a second turn and carries into it


# ---------------------------------------------------------------- the raw entry points
def test_capacities_cut_an_exact_prefix_a_graph_replays_the_eager_bits_and_the_inputs_are_never_written():
    shape = (19, 13, 37)
    valid_host, bad = ref.mask(shape)
    rec = ref.with_bad(redistance_ref.smooth_field(shape), bad)
    want = restated(rec, valid_host)
    nv, nf = want.counts
    assert nv > 1000 and nf > 1000
    lib = _lib.load()
    desc = surface_module.lattice_desc(shape, RES, ORIGIN)
    n = shape[0] * shape[1] * shape[2]
    records = torch.from_numpy(np.array(rec)).cuda().reshape(n, 4)
    valid = torch.from_numpy(valid_host).cuda().reshape(n)
    records_before, valid_before = records.clone(), valid.clone()
    assert lib.pvamd_surface_scratch_bytes(*shape) == _lib.surface_scratch_bytes(*shape)
    scratch = _lib.scratch_buffer(_lib.surface_scratch_bytes(*shape), records.device)
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    sentinel = 0x7fc12345  # a NaN as float32
    vertices = torch.full((nv, 3), sentinel, dtype=torch.int32, device="cuda")
    normals = torch.full((nv, 3), sentinel, dtype=torch.int32, device="cuda")
    faces = torch.full((nf, 3), sentinel, dtype=torch.int32, device="cuda")

    def count():
        _lib.check(lib.pvamd_surface_count(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid), 0.0, _lib.ptr(scratch),
                                           _lib.ptr(counts), _lib.stream_ptr()), "pvamd_surface_count")

    def emit(max_vertices, max_faces):
        _lib.check(lib.pvamd_surface_emit(ctypes.byref(desc), _lib.ptr(records), _lib.ptr(valid), 0.0, _lib.ptr(scratch), max_vertices,
                                          max_faces, _lib.ptr(vertices), _lib.ptr(normals), _lib.ptr(faces), _lib.stream_ptr()),
                   "pvamd_surface_emit")

    def same(rows_v, rows_f):
        for name, t, w, rows in (("vertices", vertices, want.vertices, rows_v), ("normals", normals, want.normals, rows_v),
                                 ("faces", faces, want.faces, rows_f)):
            g = t.cpu().numpy()
            assert np.array_equal(g[:rows], ref.bits(w)[:rows]), name
            assert (g[rows:] == sentinel).all(), name  # not a byte beyond the capacity

    count()
    emit(nv // 2, nf // 2)
    torch.cuda.synchronize()
    assert counts.tolist() == [nv, nf]
    same(nv // 2, nf // 2)
    half = restated(rec, valid_host, max_vertices=nv // 2, max_faces=nf // 2)  # the restatement cuts the same prefix
    assert np.array_equal(ref.bits(half.vertices[:nv // 2]), ref.bits(want.vertices[:nv // 2])) and half.counts == want.counts
    assert np.array_equal(half.faces[:nf // 2], want.faces[:nf // 2])
    emit(nv, nf)  # the scratch count left serves a second emit
    torch.cuda.synchronize()
    same(nv, nf)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        count()
        emit(nv, nf)
    for t in (vertices, normals, faces):
        t.fill_(sentinel)  # what the capture itself ran, if anything, is forgotten
    counts.zero_()
    scratch.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert counts.tolist() == [nv, nf]
    same(nv, nf)
    assert torch.equal(records.view(torch.int32), records_before.view(torch.int32)) and torch.equal(valid, valid_before)


def test_argument_errors_of_the_entry_points_launch_nothing():
    lib = _lib.load()
    E_NULL, E_ALIGN = _lib.H["PVAMD_E_NULL"], _lib.H["PVAMD_E_ALIGN"]
    shape = (5, 3, 131)
    n = 5 * 3 * 131
    desc = surface_module.lattice_desc(shape, RES, ORIGIN)
    records = torch.ones((n * 4 + 4,), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((_lib.surface_scratch_bytes(*shape) + 4,), dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    out = torch.zeros((64,), dtype=torch.float32, device="cuda")
    good = dict(records=_lib.ptr(records), valid=None, level=0.0, scratch=_lib.ptr(scratch), counts=_lib.ptr(counts))

    def count(**changes):
        return lib.pvamd_surface_count(ctypes.byref(desc), *{**good, **changes}.values(), _lib.stream_ptr())

    for name in ("records", "scratch", "counts"):
        assert count(**{name: None}) == E_NULL, name
    assert count(records=_lib.ptr(records[2:])) == E_ALIGN and count(scratch=_lib.ptr(scratch[3:])) == E_ALIGN
    assert count(counts=_lib.ptr(counts.view(torch.int32)[1:])) == E_ALIGN
    emit = dict(records=_lib.ptr(records), valid=None, level=0.0, scratch=_lib.ptr(scratch), max_vertices=4, max_faces=4,
                vertices=_lib.ptr(out), normals=None, faces=_lib.ptr(out[32:]))
    for name in ("records", "scratch", "vertices", "faces"):
        assert lib.pvamd_surface_emit(ctypes.byref(desc), *{**emit, name: None}.values(), _lib.stream_ptr()) == E_NULL, name
    for name in ("vertices", "normals", "faces"):
        off = _lib.ptr(out.view(torch.uint8)[2:])
        assert lib.pvamd_surface_emit(ctypes.byref(desc), *{**emit, name: off}.values(), _lib.stream_ptr()) == E_ALIGN, name
    torch.cuda.synchronize()
    assert (counts == -7).all() and not scratch.any() and not out.any()  # nothing was launched
    assert count(scratch=_lib.ptr(scratch[4:])) == 0  # scratch only 4-byte aligned
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, -7]  # a constant field: no crossing


# ---------------------------------------------------------------- through the volume and the cache
R, BALL_RES, TRUNC, INTRINSICS = 0.3, 0.02, 0.06, (150.0, 150.0, 79.5, 59.5)


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
def test_a_volume_meshes_to_the_restatement_on_its_own_records_and_weight_mask(min_weight):
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, INTRINSICS, 120, 160, (0.0, 0.0, 0.0), R)
    vol = pv.TSDFVolume(BALL_RES, [(-0.5, 0.5)] * 3, truncation=TRUNC, device="cuda")
    assert vol.shape == (51, 51, 51)
    vol.integrate(torch.from_numpy(depth), INTRINSICS, torch.from_numpy(poses))
    got = vol.extract_mesh(min_weight=min_weight)
    records = pv.TSDFField(vol, min_weight=min_weight)._records.cpu().numpy().reshape(51, 51, 51, 4)
    valid = (vol.weight > min_weight).cpu().numpy().astype(np.uint8)
    lat = tsdf_ref.lattice_of(vol._grid.voxels._grid_desc())
    want = ref.extract(records, valid, [lat.fmin[k] for k in range(3)], [lat.fres[k] for k in range(3)])
    assert_same(got, want)
    assert want.counts[0] > 500 and want.counts[1] > 500 and (valid == 0).sum() > 1000
    error = np.abs(np.linalg.norm(want.vertices.astype(np.float64), axis=1) - R) / BALL_RES
    assert error.max() < 1.0  # the worst crossing of this state is 0.57 voxel from the sphere (tests/test_tsdf.py)
    assert_same(vol.extract_mesh(min_weight=min_weight, normals=False),
                ref.extract(records, valid, [lat.fmin[k] for k in range(3)], [lat.fres[k] for k in range(3)], normals=False))


def test_a_cache_meshes_its_own_records_and_the_mesh_answers_like_the_ball():
    """CachedSDF -> Surface -> TriMesh -> MeshObjectFactory -> MeshSDF.  Outside the ball the mesh's distance is within 0.14 voxel of
    |c| - r: the sagitta of a chord as long as a quad's diagonal, (2 sqrt(3) h)^2 / (8 r) = 0.10 voxel, plus the vertex bound
    0.035, plus slack for float32."""
    cached = pv.CachedSDF("ball", BALL_RES, [(-0.5, 0.5)] * 3, pv.SphereSDF(R), device="cuda", cache_path=None)
    got = cached.extract_mesh()
    desc = cached._grid_desc()
    records = cached._packed.cpu().numpy().reshape(tuple(desc.shape) + (4,))
    want = ref.extract(records, None, [desc.fmin[k] for k in range(3)], [desc.fres[k] for k in range(3)])
    assert_same(got, want)
    assert want.counts == (4184, 8364)  # the analytic ball's counts (tests/test_surface.py)
    for strategy in (pv.OutOfBoundsStrategy.LOOKUP_GT_SDF, pv.OutOfBoundsStrategy.BOUNDING_BOX):
        for interpolation in ("nearest", "trilinear"):
            other = pv.CachedSDF("ball", BALL_RES, [(-0.5, 0.5)] * 3, pv.SphereSDF(R), out_of_bounds_strategy=strategy, device="cuda",
                                 cache_path=None, interpolation=interpolation)
            assert_same(other.extract_mesh(normals=False), want._replace(normals=None))
    mesh = got.to_trimesh()
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64 and mesh.faces.shape == (8364, 3)
    sdf = pv.MeshSDF(pv.MeshObjectFactory(mesh=mesh))
    rng = np.random.default_rng(6)
    direction = rng.standard_normal((400, 3))
    points = direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(R + 0.01, 0.48, size=(400, 1))
    values, _ = sdf(torch.from_numpy(points).float().cuda())
    error = (values.double().cpu().numpy() - (np.linalg.norm(points, axis=1) - R)) / BALL_RES
    print(f"mesh distance against the ball, in voxels: {error.min():+.4f} to {error.max():+.4f}")
    assert np.abs(error).max() <= 0.14
    with pytest.raises(TypeError):
        cached.extract_mesh(normals=1)
    with pytest.raises(ValueError):
        cached.extract_mesh(level=float("nan"))


class CircleSDF(pv.ObjectFrameSDF):
    """Planar ground truth: a circle of radius r at the origin."""

    def __init__(self, r):
        self.r = r

    def __call__(self, p):
        n = torch.linalg.norm(p, dim=-1)
        return n - self.r, p / (n.unsqueeze(-1) + 1e-12)

    def surface_bounding_box(self, padding=0., padding_ratio=0.):
        e = self.r + padding + padding_ratio * self.r
        return torch.tensor([[-e, e], [-e, e]])


def test_a_planar_cache_has_no_mesh():
    planar = pv.CachedSDF("circle", 0.05, [(-0.5, 0.5), (-0.4, 0.6)], CircleSDF(0.3), device="cuda", cache_path=None)
    with pytest.raises(ValueError):
        planar.extract_mesh()
