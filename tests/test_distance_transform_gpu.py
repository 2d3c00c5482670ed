"""GPU: pvamd_distance_transform against the brute-force C restatement of its contract (tests/distance_transform_ref.c) -- records,
sites and squared distances at every voxel, bit for bit -- and the Python layers on top: pv.distance_transform, pv.OccupancySDF,
the CachedSDF branch that takes its records, pv.cached_sdf_from_voxels, and such a cache as a leaf of the existing queries."""
import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import distance_transform_ref as ref
from tests import helpers as H

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _corner():
    occ = np.zeros((40, 40, 40), np.uint8)
    occ[0, 0, 0] = 1
    return occ


def _mirrored():
    occ = np.zeros((9, 8, 7), np.uint8)
    occ[2, 3, 3] = occ[6, 3, 3] = 1  # every voxel of the plane x = 4 is as far from one as from the other
    return occ


def _all_but_one():
    occ = np.ones((6, 5, 67), np.uint8)
    occ[3, 1, 65] = 0
    return occ


GRIDS = {
    "5x7x9@30": lambda: ref.random_grid((5, 7, 9), 0.3, 1),
    "3x17x4@50": lambda: ref.random_grid((3, 17, 4), 0.5, 2),
    "line-z13": lambda: ref.random_grid((1, 1, 13), 0.3, 3),
    "line-y70": lambda: ref.random_grid((1, 70, 1), 0.1, 4),
    "line-x70": lambda: ref.random_grid((70, 1, 1), 0.1, 5),
    "9x2x130": lambda: ref.random_grid((9, 2, 130), 0.1, 6),
    "2x3x2048": lambda: ref.random_grid((2, 3, 2048), 0.01, 7),
    "2048x1x2": lambda: ref.random_grid((2048, 1, 2), 0.01, 8),
    "23x19x37@2": lambda: ref.random_grid((23, 19, 37), 0.02, 9),
    "23x19x37@50": lambda: ref.random_grid((23, 19, 37), 0.5, 10),
    "23x19x37@98": lambda: ref.random_grid((23, 19, 37), 0.98, 11),
    "corner-40": _corner,
    "mirrored": _mirrored,
    "all-but-one": _all_but_one,
}


def gpu_transform(occ, resolution, signed):
    dt = pv.distance_transform(torch.from_numpy(occ), resolution=resolution, signed=signed)
    n = occ.size
    records = torch.cat((dt.values.reshape(n, 1), dt.gradients.reshape(n, 3)), dim=1).cpu().numpy()
    return dt, records, dt.sites.reshape(-1).cpu().numpy(), dt.squared.reshape(-1).cpu().numpy()


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_bit_for_bit_against_the_restatement(name, signed):
    occ = GRIDS[name]()
    resolution = 0.037
    want_rec, want_sites, want_sq = ref.transform(occ, resolution, signed)
    dt, rec, sites, sq = gpu_transform(occ, resolution, signed)
    assert dt.values.shape == occ.shape and dt.gradients.shape == occ.shape + (3,) and dt.values.is_cuda
    assert dt.values.dtype == dt.gradients.dtype == torch.float32 and dt.sites.dtype == dt.squared.dtype == torch.int32
    assert np.array_equal(sq, want_sq), int((sq != want_sq).sum())
    assert np.array_equal(sites, want_sites), int((sites != want_sites).sum())
    assert np.array_equal(bits(rec), bits(want_rec)), int((bits(rec) != bits(want_rec)).any(axis=1).sum())
    if name == "mirrored" and signed:
        plane = np.arange(occ.size).reshape(occ.shape)[4].reshape(-1)
        assert (sites[plane] == np.ravel_multi_index((2, 3, 3), occ.shape)).all()  # the smaller flat index of the two


# Past both launch caps (tests/test_launch_bounds.py): the y and x passes give a lane a second voxel above H.STREAM_GRID_ITEMS
# voxels, and the z pass gives a wave a second line -- reusing its LDS bit set -- above H.STREAM_GRID_ITEMS / 64 lines.  The
# restatement is O(voxels x sites), so these grids are nearly empty or nearly full: (name, shape, fraction, seed, signed).
LARGE_GRIDS = [
    ("100x100x70@0.1-signed", (100, 100, 70), 0.001, 51, True),    # 10,000 lines of two bit-set words with a 6-bit tail
    ("100x100x70@0.1-unsigned", (100, 100, 70), 0.001, 51, False),
    ("100x100x70@99.9-signed", (100, 100, 70), 0.999, 52, True),
    ("128x128x36@0.1-signed", (128, 128, 36), 0.001, 53, True),    # 16,384 lines: every wave takes exactly two
]


@pytest.mark.parametrize("name,shape,fraction,seed,signed", LARGE_GRIDS, ids=[g[0] for g in LARGE_GRIDS])
def test_bit_for_bit_past_the_launch_caps(name, shape, fraction, seed, signed):
    lines = shape[0] * shape[1]
    assert lines > H.STREAM_GRID_ITEMS // 64, "the z pass must take a second line per wave"
    if shape[2] == 70:
        assert lines * shape[2] > H.STREAM_GRID_ITEMS, "the y and x passes must take a second voxel per lane"
    else:
        assert lines == 2 * (H.STREAM_GRID_ITEMS // 64)
    occ = ref.random_grid(shape, fraction, seed)
    resolution = 0.037
    want_rec, want_sites, want_sq = ref.transform(occ, resolution, signed)
    rc, rec, sites, sq = c_entry(occ, resolution, signed)  # outputs pre-filled with -7: an unwritten tail fails below
    assert rc == 0
    assert np.array_equal(sq, want_sq), int((sq != want_sq).sum())
    assert np.array_equal(sites, want_sites), int((sites != want_sites).sum())
    assert np.array_equal(bits(rec), bits(want_rec)), int((bits(rec) != bits(want_rec)).any(axis=1).sum())
    dt, rec2, sites2, sq2 = gpu_transform(occ, resolution, signed)  # and the Python layer hands the same bits on
    assert np.array_equal(sq2, sq) and np.array_equal(sites2, sites) and np.array_equal(bits(rec2), bits(rec))


def test_a_graph_replay_past_the_launch_caps_gives_the_eager_bits():
    occ = torch.from_numpy(ref.random_grid((100, 100, 70), 0.001, 51)).cuda()
    assert occ.numel() > H.STREAM_GRID_ITEMS and occ.shape[0] * occ.shape[1] > H.STREAM_GRID_ITEMS // 64
    eager = pv.distance_transform(occ, resolution=0.037)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = pv.distance_transform(occ, resolution=0.037)
    for t in captured:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, captured):
        raw = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(raw(a), raw(c))
    assert (eager.squared > 0).any()


def test_input_dtypes_mean_the_same_occupancy():
    occ = ref.random_grid((6, 9, 70), 0.2, 21)
    base = gpu_transform(occ, 0.5, True)[1:]
    for t in (torch.from_numpy(occ != 0), torch.from_numpy(occ).float() * -2.5, torch.from_numpy(occ).to(torch.int64) * 7,
              torch.from_numpy(occ).cuda()):
        dt = pv.distance_transform(t, resolution=0.5)
        assert np.array_equal(dt.sites.reshape(-1).cpu().numpy(), base[1])
        assert np.array_equal(bits(dt.values.reshape(-1).cpu().numpy()), bits(base[0][:, 0]))


def c_entry(occ, resolution, signed, want_sites=True):
    """One direct call of the C entry point: (rc, records, sites, squared)."""
    lib = _lib.load()
    dev = _lib.require_gpu()
    nx, ny, nz = occ.shape
    n = occ.size
    o = torch.from_numpy(np.ascontiguousarray(occ)).to(dev)
    records = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    sites = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_sites else None
    squared = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_sites else None
    scratch = _lib.scratch_buffer(max(1, lib.pvamd_distance_transform_scratch_bytes(nx, ny, nz, int(signed))), dev)
    rc = lib.pvamd_distance_transform(_lib.ptr(o), nx, ny, nz, resolution, int(signed), _lib.ptr(records), _lib.ptr(sites),
                                      _lib.ptr(squared), _lib.ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, records.cpu().numpy(), None if sites is None else sites.cpu().numpy(), None if squared is None else squared.cpu().numpy()


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_empty_site_classes_give_the_sentinels(signed):
    shape = (5, 3, 70)
    rc, rec, sites, sq = c_entry(np.zeros(shape, np.uint8), 0.5, signed)
    assert rc == 0
    assert (sq == _lib.EDT_NO_SITE).all() and (sites == -1).all()
    assert np.array_equal(bits(rec), bits(np.tile(np.array([np.inf, 0, 0, 0], np.float32), (rec.shape[0], 1))))
    rc, rec, sites, sq = c_entry(np.ones(shape, np.uint8), 0.5, signed)
    assert rc == 0
    if signed:
        assert (sq == _lib.EDT_NO_SITE).all() and (sites == -1).all()
        assert np.array_equal(bits(rec), bits(np.tile(np.array([-np.inf, 0, 0, 0], np.float32), (rec.shape[0], 1))))
    else:  # every voxel is its own site
        assert (sq == 0).all() and np.array_equal(sites, np.arange(sites.size))
        assert np.array_equal(bits(rec), np.zeros(rec.shape, np.int32))
    want = ref.transform(np.ones(shape, np.uint8), 0.5, signed)
    assert np.array_equal(bits(rec), bits(want[0])) and np.array_equal(sites, want[1]) and np.array_equal(sq, want[2])


def test_sites_and_squared_are_optional_and_shape_errors_are_refused():
    occ = ref.random_grid((7, 6, 66), 0.15, 31)
    rc, rec, sites, sq = c_entry(occ, 0.25, True)
    rc2, rec2, none_sites, none_sq = c_entry(occ, 0.25, True, want_sites=False)
    assert rc == rc2 == 0 and none_sites is None and none_sq is None
    assert np.array_equal(bits(rec), bits(rec2)) and np.array_equal(bits(rec), bits(ref.transform(occ, 0.25, True)[0]))
    lib = _lib.load()
    buf = torch.zeros((64,), dtype=torch.float32, device="cuda")
    for shape in ((2049, 1, 1), (1, 2049, 1), (1, 1, 2049), (0, 1, 1)):
        assert lib.pvamd_distance_transform(_lib.ptr(buf), *shape, 1.0, 1, _lib.ptr(buf), None, None, _lib.ptr(buf), _lib.stream_ptr()) \
            == _lib.E_SHAPE, shape
    with pytest.raises(ValueError):
        pv.distance_transform(torch.zeros((2, 2049, 2), device="cuda"))
    torch.cuda.synchronize()


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    occ = torch.from_numpy(ref.random_grid((19, 23, 70), 0.05, 41)).cuda()
    first = pv.distance_transform(occ, resolution=0.02)
    second = pv.distance_transform(occ, resolution=0.02)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = pv.distance_transform(occ, resolution=0.02)
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, captured):
        raw = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(a), raw(c))
    assert (first.squared > 0).any()


# ---------------------------------------------------------------- OccupancySDF, the CachedSDF branch, cached_sdf_from_voxels
def blob_grid(ranges, resolution=0.05, dtype=torch.float):
    """A VoxelGrid on the GPU with two overlapping balls of voxels set (values 1 and 3) and the rest unknown."""
    grid = pv.VoxelGrid(resolution, ranges, dtype=dtype, device="cuda")
    pts = grid.get_voxel_center_points()
    a = (pts - torch.tensor([0.05, 0.0, 0.05], device="cuda")).norm(dim=-1) <= 0.17
    b = (pts - torch.tensor([-0.1, 0.1, 0.0], device="cuda")).norm(dim=-1) <= 0.11
    grid[pts[a]] = 1
    grid[pts[b & ~a]] = 3
    return grid


RANGES = {"float64-range": np.array([[-0.4, 0.45], [-0.3, 0.3], [-0.25, 0.35]]),
          "float32-range": [(-0.4, 0.45), (-0.3, 0.3), (-0.25, 0.35)]}


def query_points(field, dtype):
    """Points inside the lattice, on its faces and corners, at voxel centres and up to 0.2 outside."""
    lo = np.array([float(r[0]) for r in field.ranges])
    hi = np.array([float(r[1]) for r in field.ranges])
    cloud = H.uniform_points(4000, lo - 0.2, hi + 0.2, seed=5).double()
    faces = H.uniform_points(600, lo, hi, seed=6).double()
    for k in range(600):
        faces[k, k % 3] = (lo if (k // 3) % 2 else hi)[k % 3]
    corners = torch.tensor([[a, b, c] for a in (lo[0], hi[0]) for b in (lo[1], hi[1]) for c in (lo[2], hi[2])], dtype=torch.float64)
    coords, centres = pv.get_coordinates_and_points_in_grid(field.resolution, field.ranges)
    return torch.cat((cloud, faces, corners, centres[::7].double())).to(dtype)


@pytest.fixture(scope="module", params=list(RANGES))
def field_and_cache(request):
    grid = blob_grid(RANGES[request.param])
    field = pv.OccupancySDF(grid)
    cached = pv.CachedSDF("blob", field.resolution, field.ranges, field, device="cuda", cache_path=None)
    return request.param, grid, field, cached


def test_field_and_cache_over_the_same_lattice_are_the_same_bits(field_and_cache):
    kind, grid, field, cached = field_and_cache
    assert cached._view.index_f64 == field._view.index_f64 == (kind == "float64-range")
    assert cached._view.shape == tuple(grid.get_voxel_values().shape) == (18, 13, 13)
    dt = pv.distance_transform(grid.get_voxel_values() != 0, resolution=grid.resolution, signed=True)
    n = cached._packed.shape[0]
    assert cached._packed.data_ptr() != field._records.data_ptr()
    assert torch.equal(cached._packed.view(torch.int32), field._records.view(torch.int32))
    assert torch.equal(cached._packed[:, 0].view(torch.int32), dt.values.reshape(n).view(torch.int32))
    assert torch.equal(cached._packed[:, 1:].contiguous().view(torch.int32), dt.gradients.reshape(n, 3).contiguous().view(torch.int32))
    box = field.surface_bounding_box()
    assert box.dtype == torch.float64 and box.shape == (3, 2) and torch.equal(box, cached.surface_bounding_box())
    for dtype in (torch.float32, torch.float64):
        pts = query_points(field, dtype)
        fv, fg = field(pts)
        cv, cg = cached(pts.cuda())
        assert fv.dtype == dtype and fv.device == pts.device and fv.shape == pts.shape[:-1] and fg.shape == pts.shape
        assert not fv.requires_grad and not fg.requires_grad
        assert torch.equal(fv, cv.cpu()) and torch.equal(fg, cg.cpu())
        assert torch.isfinite(fv).all() and (fv > 0).any() and (fv < 0).any()


def test_bounding_box_is_the_box_of_the_occupied_cubes(field_and_cache):
    _, grid, field, _ = field_and_cache
    pos, _ = grid.get_known_pos_and_values()
    pos = pos.double().cpu()
    half = grid.resolution / 2
    box = field.surface_bounding_box()
    assert torch.allclose(box[:, 0], pos.amin(dim=0) - half, atol=1e-6) and torch.allclose(box[:, 1], pos.amax(dim=0) + half, atol=1e-6)
    padded = field.surface_bounding_box(padding=0.1, padding_ratio=0.5)
    ext = box[:, 1] - box[:, 0]
    assert torch.equal(padded, torch.stack((box[:, 0] - (0.1 + 0.5 * ext), box[:, 1] + (0.1 + 0.5 * ext)), dim=1))


def test_cache_on_another_lattice_asks_the_field_at_its_centres(field_and_cache):
    _, _, field, _ = field_and_cache
    fine = pv.CachedSDF("blob-fine", field.resolution / 2, field.ranges, field, device="cuda", cache_path=None)
    assert fine._view.shape != field._view.shape
    _, centres = pv.get_coordinates_and_points_in_grid(fine.resolution, fine.ranges)
    val, grad = field(centres.cuda())
    assert torch.equal(fine._packed[:, 0], val) and torch.equal(fine._packed[:, 1:], grad)


def test_threshold_unsigned_and_construction_errors():
    grid = blob_grid(RANGES["float32-range"])
    ones = pv.VoxelGrid(0.05, RANGES["float32-range"], device="cuda")
    pos, val = grid.get_known_pos_and_values()
    ones[pos[val > 2]] = 1
    a, b = pv.OccupancySDF(grid, threshold=2), pv.OccupancySDF(ones)
    assert torch.equal(a._records.view(torch.int32), b._records.view(torch.int32)) and torch.equal(a._sites, b._sites)
    unsigned = pv.OccupancySDF(grid, signed=False)
    assert (unsigned._records[:, 0] >= 0).all() and (unsigned._records[:, 0] == 0).sum() == (grid.get_voxel_values() != 0).sum()
    empty = pv.VoxelGrid(0.05, RANGES["float32-range"], device="cuda")
    with pytest.raises(ValueError, match="no occupied"):
        pv.OccupancySDF(empty)
    with pytest.raises(ValueError, match="no occupied"):
        pv.OccupancySDF(grid, threshold=5)
    empty.get_voxel_values().fill_(1)
    with pytest.raises(ValueError, match="free voxel"):
        pv.OccupancySDF(empty)
    assert pv.OccupancySDF(empty, signed=False)._records.abs().max() == 0
    with pytest.raises(ValueError):
        pv.OccupancySDF(pv.VoxelGrid(0.05, [(0.0, 1.0), (0.0, 1.0)], device="cuda"))


# ---------------------------------------------------------------- a voxelised ball as a leaf of the existing queries
@pytest.fixture(scope="module")
def ball_scene():
    grid = pv.VoxelGrid(ref.BALL_RES, ref.BALL_RANGE, device="cuda")
    centres = grid.get_voxel_center_points()
    grid[centres[centres.norm(dim=-1) <= ref.BALL_RADIUS]] = 1
    return grid, pv.cached_sdf_from_voxels("ball", grid)


def unit_directions(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn((n, 3), generator=g, dtype=torch.float64)
    return (d / d.norm(dim=-1, keepdim=True)).float()


def test_cached_sdf_from_voxels_is_the_two_lines_and_follows_the_ball(ball_scene):
    grid, scene = ball_scene
    assert isinstance(scene, pv.CachedSDF) and isinstance(scene.gt_sdf, pv.OccupancySDF) and scene._view.shape == (51, 51, 51)
    assert scene.interpolation == "nearest" and scene.out_of_bounds_strategy == pv.OutOfBoundsStrategy.BOUNDING_BOX
    assert torch.equal(scene._packed.view(torch.int32), scene.gt_sdf._records.view(torch.int32))
    centres = grid.get_voxel_center_points()
    # the interval of tests/test_distance_transform.py: a voxel centre lies within (sqrt(3) / 2) res of any point
    err = scene._packed[:, 0].double() - (centres.double().norm(dim=-1) - ref.BALL_RADIUS)
    free = (grid.get_voxel_values() == 0).reshape(-1)
    lo, hi = -0.5 * ref.BALL_RES - 1e-5, (np.sqrt(3) - 0.5) * ref.BALL_RES + 1e-5
    assert (err[free] >= lo).all() and (err[free] <= hi).all() and (err[~free] >= -hi).all() and (err[~free] <= -lo).all()
    smooth = pv.cached_sdf_from_voxels("ball", grid, interpolation="trilinear")
    inner = centres[(centres.abs() < 0.45).all(dim=-1)][::11]
    assert torch.allclose(smooth(inner)[0], scene(inner)[0], atol=1e-6)  # at the lattice nodes both read the node
    off = inner + 0.004
    # a blend of nodes at most sqrt(3) res away, each within the interval above of its own distance
    assert (smooth(off)[0] - (off.double().norm(dim=-1) - ref.BALL_RADIUS).float()).abs().max() <= (2 * np.sqrt(3) - 0.5) * ref.BALL_RES


def test_expanding_grid_written_through_points():
    grid = pv.ExpandingVoxelGrid(ref.BALL_RES, [(-0.1, 0.1)] * 3, device="cuda")
    surface = unit_directions(4000, seed=3).cuda() * 0.25
    grid[surface] = 1
    scene = pv.cached_sdf_from_voxels("shell", grid, signed=False)
    assert min(scene._view.shape) >= 25
    val, _ = scene(surface)
    assert (val == 0).all()  # every written point lies in an occupied voxel
    assert scene(torch.zeros((1, 3), device="cuda"))[0].item() == pytest.approx(0.25, abs=ref.BALL_RES * 1.8)


def test_composition_with_a_mesh_cache_is_fused_and_the_minimum_of_its_leaves():
    grid = pv.VoxelGrid(ref.BALL_RES, ref.BALL_RANGE, device="cuda")
    centres = grid.get_voxel_center_points()
    grid[centres[(centres - torch.tensor([0.3, 0.1, 0.0], device="cuda")).norm(dim=-1) <= 0.12]] = 1  # beside the drill, not around it
    scene = pv.cached_sdf_from_voxels("scene", grid)
    obj = pv.MeshObjectFactory(H.mesh_path("ycb_power_drill.npz"))
    drill = pv.CachedSDF("drill", 0.01, obj.bounding_box(padding=0.1), pv.MeshSDF(obj), device="cuda", cache_path=None)
    comp = pv.ComposedSDF([drill, scene], torch.eye(4).repeat(2, 1, 1))
    assert comp._fusable()
    pts = H.uniform_points(20_000, np.full(3, -0.7), np.full(3, 0.7), seed=9).cuda()
    val, grad = comp(pts)
    dv, dg = drill(pts)
    sv, sg = scene(pts)
    assert torch.equal(val.reshape(-1), torch.minimum(dv, sv))
    assert torch.equal(grad.reshape(-1, 3), torch.where((sv < dv).unsqueeze(-1), sg, dg))  # the first minimum: the drill on a tie
    assert (sv < dv).any() and (dv < sv).any()


def test_rays_aimed_at_the_ball_hit_it(ball_scene):
    _, scene = ball_scene
    d = unit_directions(2000, seed=1).cuda()
    for start in (0.45, 0.8):  # inside the lattice, and outside it where the bounding-box distance answers
        res = scene.ray_cast(-d * start, d, t_max=2.0)
        assert (res.status == pv.RAY_HIT).all()
        hit = (-d * start + res.t.unsqueeze(-1) * d).norm(dim=-1)
        # the hit lies in an occupied voxel, and the last step is at most the distance to the nearest occupied centre minus half a
        # voxel, taken from a point within (sqrt(3) / 2) res of its own centre: no deeper than 0.5 + 3 sqrt(3) / 2 - 1 = 2.1 res
        assert (hit <= ref.BALL_RADIUS + ref.BALL_RES).all() and (hit >= ref.BALL_RADIUS - 3 * ref.BALL_RES).all()


def test_pose_refinement_against_the_ball_never_increases_the_cost(ball_scene):
    _, scene = ball_scene
    pts = unit_directions(600, seed=2).cuda() * ref.BALL_RADIUS
    W = H.random_rigid(6, seed=4, trans=0.05).cuda()
    res = pv.refine_poses(W, pts, scene, iterations=6)
    assert torch.isfinite(res.cost).all() and (res.cost <= res.initial_cost).all() and (res.accepted >= 1).all()
