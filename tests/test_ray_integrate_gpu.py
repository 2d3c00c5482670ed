"""-m gpu: ray integration on the device, bit for bit against the C restatement of the contract (tests/ray_integrate_ref.c), through
pv.OccupancyMap and pv.ray_marks."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import helpers as H
from tests import ray_integrate_ref as ref

pytestmark = pytest.mark.gpu

# resolution 0.25 over ranges that start on a multiple of it: lattice coordinates of the ray sets' half-integers are exact
LATTICES = {(2, 2, 2): [(0.0, 0.25), (-1.0, -0.75), (0.5, 0.75)],
            (5, 7, 9): [(-0.5, 0.5), (-1.0, 0.5), (0.0, 2.0)],
            (33, 20, 65): [(-4.0, 4.0), (0.0, 4.75), (-8.0, 8.0)],
            (2, 3, 300): [(0.0, 0.25), (-0.25, 0.25), (-30.0, 44.75)]}
RAY_COUNTS = [0, 1, 63, 64, 65, 4097]


def new_map(shape, ranges=None, **kwargs):
    omap = pv.OccupancyMap(0.25, LATTICES[shape] if ranges is None else ranges, device="cuda", **kwargs)
    assert omap.shape == shape
    return omap


def lattice(omap):
    return ref.lattice_of(omap._grid.voxels._grid_desc())


@functools.lru_cache(maxsize=None)
def scene(shape, R, seed=3):
    """(origins, endpoints) of the mixed ray set on a lattice, as read-only numpy arrays shared between tests."""
    o, e = ref.mixed_rays(lattice(new_map(shape)), R, seed)
    o.flags.writeable = e.flags.writeable = False
    return o, e


def tensor(a):
    """A host tensor with its own copy of a (possibly read-only, possibly strided) numpy array."""
    return torch.from_numpy(np.array(a))


def gpu_marks(omap, o, e, max_range):
    return pv.ray_marks(omap, tensor(o), tensor(e), max_range=max_range).cpu().numpy()


# ---------------------------------------------------------------- marks
@pytest.mark.parametrize("max_range", [math.inf, 1.3])
@pytest.mark.parametrize("R", RAY_COUNTS)
@pytest.mark.parametrize("shape", list(LATTICES))
def test_marks_bit_for_bit_with_per_ray_origins(shape, R, max_range):
    omap = new_map(shape)
    o, e = scene(shape, R)
    got = gpu_marks(omap, o, e, max_range)
    assert got.shape == shape and got.dtype == np.uint8
    want = ref.mark(lattice(omap), o, e, max_range) if R else np.zeros(shape, np.uint8)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not omap.observed.any() and not omap._marks.any()  # the map is untouched


@pytest.mark.parametrize("max_range", [math.inf, 1.3])
@pytest.mark.parametrize("R", RAY_COUNTS)
@pytest.mark.parametrize("shape", list(LATTICES))
def test_marks_bit_for_bit_with_a_shared_origin_and_equal_to_the_expanded_one(shape, R, max_range):
    omap = new_map(shape)
    lat = lattice(omap)
    _, e = scene(shape, R)
    n = np.array(shape)
    for eye in (ref.world(lat, 0.37 * (n - 1)), ref.world(lat, [-2.25, 0.4 * n[1], n[2] + 1.5]), ref.world(lat, [0.5, 0.5, 0.5])):
        got = gpu_marks(omap, eye, e, max_range)  # inside, outside, on a cell corner
        want = ref.mark(lat, eye, e, max_range) if R else np.zeros(shape, np.uint8)
        assert np.array_equal(got, want), (eye, int((got != want).sum()))
        expanded = gpu_marks(omap, np.ascontiguousarray(np.broadcast_to(eye, e.shape)), e, max_range)
        assert np.array_equal(got, expanded)


def test_marks_past_the_streaming_cap():
    """More rays than the capped grid has lanes: the first 4099 lanes take a second ray."""
    shape, R = (5, 7, 9), H.PAST_CAP
    omap = new_map(shape)
    o, e = scene(shape, R, seed=9)
    lat = lattice(omap)
    assert np.array_equal(gpu_marks(omap, o, e, 1.3), ref.mark(lat, o, e, 1.3))
    # with the first turn's rays ignored, what the second turn marks is not hidden under 524,288 other rays
    sparse = e.copy()
    sparse[:H.STREAM_GRID_ITEMS] = np.nan
    tail = ref.mark(lat, o[H.STREAM_GRID_ITEMS:], e[H.STREAM_GRID_ITEMS:], 1.3)
    assert {ref.MARK_FREE, ref.MARK_HIT} <= set(np.unique(tail))
    assert np.array_equal(gpu_marks(omap, o, sparse, 1.3), tail)
    eye = ref.world(lat, [1.2, 2.3, 3.4])
    assert np.array_equal(gpu_marks(omap, eye, sparse, 1.3), ref.mark(lat, eye, e[H.STREAM_GRID_ITEMS:], 1.3))


def test_float64_ranges_index_the_hit_voxel_in_float64():
    ranges = [(np.float64(-0.5), np.float64(0.5)), (np.float64(-1.0), np.float64(0.5)), (np.float64(0.0), np.float64(2.0))]
    omap = new_map((5, 7, 9), ranges)
    assert omap._grid.voxels._grid_desc().index_f64 == 1
    o, e = scene((5, 7, 9), 4097)
    assert np.array_equal(gpu_marks(omap, o, e, math.inf), ref.mark(lattice(omap), o, e))


@pytest.mark.parametrize("shape", [(5, 7, 9), (33, 20, 65)])
def test_hit_voxels_are_the_voxel_index_of_the_endpoints_and_what_a_voxel_grid_sets(shape):
    omap = new_map(shape)
    o, e = scene(shape, 4097)
    max_range = 1.3
    marks = pv.ray_marks(omap, tensor(o), tensor(e), max_range=max_range)
    dev = tensor(e).cuda()
    flat = torch.full((len(e),), -7, dtype=torch.int64, device="cuda")
    valid = torch.zeros((len(e),), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().pvamd_voxel_index(ctypes.byref(omap._grid.voxels._grid_desc()), _lib.ptr(dev), len(e), None, _lib.ptr(flat),
                                             _lib.ptr(valid), _lib.stream_ptr()), "pvamd_voxel_index")
    finite = np.isfinite(o).all(axis=1) & np.isfinite(e).all(axis=1)
    with np.errstate(all="ignore"):
        vx, vy, vz = (e[:, k] - o[:, k] for k in range(3))  # float32, each operation rounded on its own: statement 5
        length = np.sqrt((vx * vx + vy * vy) + vz * vz)
        hits = finite & ~(length > np.float32(max_range)) & valid.cpu().numpy().astype(bool)
    assert 100 < hits.sum() < len(e) - 100
    want = np.zeros(omap.log_odds.numel(), bool)
    want[flat.cpu().numpy()[hits]] = True
    assert np.array_equal((marks == _lib.MARK_HIT).cpu().numpy().reshape(-1), want)
    grid = pv.VoxelGrid(0.25, LATTICES[shape], dtype=torch.bool, device="cuda")
    grid[dev[tensor(hits).cuda()]] = 1
    assert torch.equal(grid.get_voxel_values(), marks == _lib.MARK_HIT)


# ---------------------------------------------------------------- update
def scans(shape, count):
    """`count` scans of a fixed scene: the same endpoints seen from a few eyes in turn."""
    _, e = scene(shape, 4097)
    lat = lattice(new_map(shape))
    n = np.array(shape)
    eyes = [ref.world(lat, f * (n - 1)) for f in (0.1, 0.5, 0.8)]
    return [(eyes[i % 3], e[i % 2::2], math.inf if i % 4 else 2.0) for i in range(count)]


@pytest.mark.parametrize("count", [1, 2, 25])
def test_log_odds_and_observed_after_scans(count):
    shape = (33, 20, 65)
    omap, twin = new_map(shape), new_map(shape)
    lat = lattice(omap)
    constants = ref.log_odds_constants()
    assert (omap.l_hit, omap.l_miss, omap.l_min, omap.l_max) == tuple(float(c) for c in constants)
    want_l, want_seen, marks = np.zeros(shape, np.float32), np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for eye, e, max_range in scans(shape, count):
        for m in (omap, twin):
            m.integrate(tensor(eye), tensor(e), max_range=max_range)
            assert not m._marks.any()  # zero after every integrate
        ref.update(ref.mark(lat, eye, e, max_range, marks=marks), want_l, want_seen, *constants)
        assert not marks.any()
    got_l, got_seen = omap.log_odds.cpu().numpy(), omap.observed.cpu().numpy()
    assert np.array_equal(got_l.view(np.int32), want_l.view(np.int32)), int((got_l.view(np.int32) != want_l.view(np.int32)).sum())
    assert np.array_equal(got_seen, want_seen.astype(bool))
    assert 0 < got_seen.sum() < got_seen.size
    assert not got_l[~got_seen].view(np.int32).any()  # never touched: +0.0, bit for bit
    assert torch.equal(omap.log_odds.view(torch.int32), twin.log_odds.view(torch.int32)) and torch.equal(omap.observed, twin.observed)
    if count == 25:
        assert (got_l == constants[2]).any() and (got_l == constants[3]).any()  # both clamps reached
    assert got_l.min() >= constants[2] and got_l.max() <= constants[3]


def test_update_of_a_voxel_count_that_is_no_multiple_of_four():
    """The C entry point on n = 4 k + 1, 2, 3 voxels: the lane after the last whole group takes the rest.  The last count is past
    the streaming cap: a lane takes four voxels, so the first 4099 lanes of the capped grid take a second group."""
    lib = _lib.load()
    constants = ref.log_odds_constants()
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 1026, 4099, 4 * H.PAST_CAP + 3):
        marks = rng.integers(0, 3, size=n).astype(np.uint8)
        log_odds = rng.uniform(-2, 3.4, size=n).astype(np.float32)
        seen = rng.integers(0, 2, size=n).astype(np.uint8)
        d_marks, d_l, d_seen = (tensor(a.copy()).cuda() for a in (marks, log_odds, seen))
        rc = lib.pvamd_occupancy_update(_lib.ptr(d_marks), n, *(float(c) for c in constants), _lib.ptr(d_l), _lib.ptr(d_seen),
                                        _lib.stream_ptr())
        assert rc == 0
        ref.update(marks, log_odds, seen, *constants)
        assert not d_marks.any() and not marks.any()
        assert np.array_equal(d_l.cpu().numpy().view(np.int32), log_odds.view(np.int32)) and np.array_equal(d_seen.cpu().numpy(), seen)


def test_argument_errors_of_the_entry_points():
    lib = _lib.load()
    omap = new_map((5, 7, 9))
    desc = omap._grid.voxels._grid_desc()
    buf = torch.zeros((5 * 7 * 9 * 4,), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    call = lambda *a: lib.pvamd_ray_mark(*a, _lib.stream_ptr())
    assert call(ctypes.byref(desc), _lib.ptr(pts), 0, _lib.ptr(pts), -1, math.inf, _lib.ptr(buf)) == _lib.E_SHAPE
    assert call(None, _lib.ptr(pts), 0, _lib.ptr(pts), 4, math.inf, _lib.ptr(buf)) == _lib.H["PVAMD_E_NULL"]
    assert call(ctypes.byref(desc), None, 0, _lib.ptr(pts), 4, math.inf, _lib.ptr(buf)) == _lib.H["PVAMD_E_NULL"]
    assert call(ctypes.byref(desc), _lib.ptr(pts), 0, _lib.ptr(pts), 4, math.inf, None) == _lib.H["PVAMD_E_NULL"]
    for bad in (math.nan, 0.0, -1.0):
        assert call(ctypes.byref(desc), _lib.ptr(pts), 0, _lib.ptr(pts), 4, bad, _lib.ptr(buf)) == _lib.H["PVAMD_E_MODE"]
    assert call(ctypes.byref(desc), _lib.ptr(pts), 2, _lib.ptr(pts), 4, 1.0, _lib.ptr(buf)) == _lib.H["PVAMD_E_MODE"]
    wide = _lib.GridDesc.from_buffer_copy(desc)
    wide.shape[2] = 2049
    assert call(ctypes.byref(wide), _lib.ptr(pts), 0, _lib.ptr(pts), 4, math.inf, _lib.ptr(buf)) == _lib.E_SHAPE
    update = lambda *a: lib.pvamd_occupancy_update(*a, _lib.stream_ptr())
    l = torch.zeros((64,), dtype=torch.float32, device="cuda")
    assert update(_lib.ptr(buf), -1, 0.8, -0.4, -2.0, 3.5, _lib.ptr(l), None) == _lib.E_SHAPE
    assert update(_lib.ptr(buf), 64, 0.8, -0.4, 3.5, -2.0, _lib.ptr(l), None) == _lib.H["PVAMD_E_MODE"]
    assert update(_lib.ptr(buf), 64, math.nan, -0.4, -2.0, 3.5, _lib.ptr(l), None) == _lib.H["PVAMD_E_MODE"]
    assert update(None, 64, 0.8, -0.4, -2.0, 3.5, _lib.ptr(l), None) == _lib.H["PVAMD_E_NULL"]
    assert update(_lib.ptr(buf), 64, 0.8, -0.4, -2.0, 3.5, None, None) == _lib.H["PVAMD_E_NULL"]
    assert update(_lib.ptr(buf), 60, 0.8, -0.4, -2.0, 3.5, _lib.ptr(l[1:]), None) == _lib.H["PVAMD_E_ALIGN"]
    assert update(_lib.ptr(buf[1:]), 60, 0.8, -0.4, -2.0, 3.5, _lib.ptr(l), None) == _lib.H["PVAMD_E_ALIGN"]
    assert update(_lib.ptr(buf), 64, 0.8, -0.4, -2.0, 3.5, _lib.ptr(l), None) == 0  # observed is optional
    torch.cuda.synchronize()
    assert not l.any() and not buf.any()


# ---------------------------------------------------------------- carving, unknown space, the SDF
def test_carving_frees_a_voxel_an_earlier_scan_set_and_the_sdf_follows():
    shape = (33, 20, 65)
    omap = new_map(shape)
    lat = lattice(omap)
    eye = ref.world(lat, [2.0, 10.0, 30.0])
    target = (16, 10, 30)
    omap.integrate(tensor(eye), tensor(ref.world(lat, [target])))
    assert omap.log_odds[target] > 0 and omap.occupied()[target] and omap.observed[target]
    before = omap.to_sdf("before")
    twin = pv.VoxelGrid(0.25, LATTICES[shape], dtype=torch.bool, device="cuda")
    twin.get_voxel_values().copy_(omap.occupied())
    same = pv.cached_sdf_from_voxels("twin", twin)
    assert torch.equal(before._packed.view(torch.int32), same._packed.view(torch.int32))
    # later scans look through the voxel at a wall behind it
    wall = ref.world(lat, [[30.0, y, z] for y in (9.0, 10.0, 11.0) for z in (29.0, 30.0, 31.0)])
    scans_needed = 0
    while omap.log_odds[target] >= 0:
        omap.integrate(tensor(eye), tensor(wall))
        scans_needed += 1
        assert scans_needed <= 3  # 0.847 / 0.405: the third crossing takes it below zero
    assert scans_needed == 3
    assert omap.log_odds[target] < 0 and not omap.occupied()[target] and omap.observed[target]
    assert omap.occupied()[30, 10, 30]
    after = omap.to_sdf("after")
    flat = (target[0] * shape[1] + target[1]) * shape[2] + target[2]
    assert before._packed[flat, 0] < 0 < after._packed[flat, 0]
    probe = tensor(ref.world(lat, [target])).cuda()
    assert before(probe)[0] < 0 < after(probe)[0]
    omap.reset()
    assert not omap.observed.any() and not omap.log_odds.view(torch.int32).any() and not omap._marks.any()


def test_unknown_occupied_counts_never_observed_voxels():
    omap = new_map((33, 20, 65))
    eye, e, max_range = scans((33, 20, 65), 1)[0]
    omap.integrate(tensor(eye), tensor(e), max_range=max_range)
    plain, wary = omap.occupied(), omap.occupied(unknown="occupied")
    assert torch.equal(wary, plain | ~omap.observed)
    assert plain.any() and (wary & ~plain).any() and not wary.all()
    assert torch.equal(plain, omap.probability() > 0.5)
    assert torch.equal(omap.occupied(threshold=0.3), (omap.probability() > 0.3) & omap.observed)
    wary_sdf, plain_sdf = omap.to_sdf("wary", unknown="occupied"), omap.to_sdf("plain")
    assert (wary_sdf._packed[:, 0] <= plain_sdf._packed[:, 0]).all() and (wary_sdf._packed[:, 0] < plain_sdf._packed[:, 0]).any()


def test_a_leading_shape_and_broadcast_origins_are_one_scan():
    shape = (5, 7, 9)
    omap = new_map(shape)
    o, e = scene(shape, 4096)
    image = tensor(e).reshape(64, 64, 3)
    eyes = tensor(o[:64].copy()).reshape(64, 1, 3)
    got = pv.ray_marks(omap, eyes, image).cpu().numpy()
    want = ref.mark(lattice(omap), np.repeat(o[:64], 64, axis=0), e)
    assert np.array_equal(got, want)
    got64 = pv.ray_marks(omap, eyes.double(), image.double()).cpu().numpy()  # cast to float32 on the way in
    assert np.array_equal(got64, want)


# ---------------------------------------------------------------- graph capture
def test_two_replays_of_a_captured_integrate_equal_two_eager_calls():
    shape = (33, 20, 65)
    eye, e, _ = scans(shape, 1)[0]
    eye_dev, e_dev = tensor(eye).cuda(), tensor(e).cuda().contiguous()
    eager, captured = new_map(shape), new_map(shape)
    for _ in range(2):
        eager.integrate(eye_dev, e_dev, max_range=3.0)
    captured.integrate(eye_dev, e_dev, max_range=3.0)  # warm: the library and its kernels are loaded before the capture
    captured.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.integrate(eye_dev, e_dev, max_range=3.0)
    captured.reset()  # what the capture itself ran, if anything, is forgotten
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert eager.observed.any()
    assert torch.equal(eager.log_odds.view(torch.int32), captured.log_odds.view(torch.int32))
    assert torch.equal(eager.observed, captured.observed) and not captured._marks.any()
