"""-m gpu: the volume kernels (csrc/ray_integrate.hip, tsdf.hip, redistance.hip) bit for bit against their C restatements on
lattices whose arithmetic rounds -- a fine one off the origin, one near +/-1000 where a float32 step is three thousandths of a
voxel, the same indexed in float64 -- and on axes of PVAMD_LATTICE_MAX_AXIS voxels.  The sibling files use resolution 0.25 or
0.5 over ranges that start on a multiple of it, where a fused multiply-add or a reciprocal gives the same bits as the contract's
statements; here they do not.  tests/test_volume_lattices.py ties the restatements to float64 references."""
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from tests import ray_integrate_ref as rays
from tests import redistance_ref as redist
from tests import tsdf_ref
from tests import volume_truth as truth

pytestmark = pytest.mark.gpu

RES = {"fine": 0.013, "far": 0.02, "far64": 0.02, "limit": 0.02}
LOW = {"fine": (3.37, -1.21, 0.113), "far": (1000.37, -998.21, 500.113),
       "far64": (np.float64(1000.37), np.float64(-998.21), np.float64(500.113)), "limit": (3.37, -1.21, -20.0)}
RAY_LATTICES = [("fine", (19, 13, 37)), ("fine", (33, 20, 65)), ("far", (5, 3, 131)), ("far", (5, 7, 9)),
                ("far64", (5, 3, 131)), ("far64", (5, 7, 9))]
TSDF_LATTICES = [("fine", (19, 13, 37)), ("far", (5, 3, 131))]
LIMIT_SHAPES = [(2048, 2, 3), (2, 2048, 3), (3, 2, 2048)]  # limit-x, limit-y, limit-z
INTRINSICS = (40.0, 36.0, 31.5, 23.5)
MAX_DEPTH = 500.0
BANDS = {"smooth": 0.4, "tie": 25.0, "half": 0.0}


def ranges_of(name, shape):
    """(low, low + (n - 1) * res) per axis: round(span / res) + 1 is not near a half, and the shape is the one intended."""
    return [(low, low + (n - 1) * RES[name]) for low, n in zip(LOW[name], shape)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def tensor(a):
    return torch.from_numpy(np.array(a))


# ---------------------------------------------------------------- rays
def new_map(name, shape):
    omap = pv.OccupancyMap(RES[name], ranges_of(name, shape), device="cuda")
    assert omap.shape == shape and omap._grid.voxels._grid_desc().index_f64 == (name == "far64")
    return omap


def ray_lattice(omap):
    return rays.lattice_of(omap._grid.voxels._grid_desc())


def gpu_marks(omap, o, e, max_range):
    return pv.ray_marks(omap, tensor(o), tensor(e), max_range=max_range).cpu().numpy()


def eyes_of(lat):
    """A shared origin inside the grid and one outside it."""
    n = np.array(lat.dims)
    return rays.world(lat, 0.37 * (n - 1)), rays.world(lat, [-2.25, 0.4 * n[1], n[2] + 1.5])


@pytest.mark.parametrize("R", [65, 4097])
@pytest.mark.parametrize("name, shape", RAY_LATTICES)
def test_marks_bit_for_bit_where_lattice_coordinates_round(name, shape, R):
    omap = new_map(name, shape)
    lat = ray_lattice(omap)
    o, e = rays.mixed_rays(lat, R, seed=3)
    for max_range in (math.inf, 40 * RES[name]):
        for origins in (o,) + eyes_of(lat):  # per ray, shared inside, shared outside
            got, want = gpu_marks(omap, origins, e, max_range), rays.mark(lat, origins, e, max_range)
            assert np.array_equal(got, want), (max_range, origins.shape, int((got != want).sum()))
            assert R < 1000 or {rays.MARK_FREE, rays.MARK_HIT} <= set(np.unique(want))


@pytest.mark.parametrize("name, shape", [("fine", (33, 20, 65)), ("far", (5, 7, 9)), ("far64", (5, 7, 9))])
def test_one_integrate_of_two_scans_where_lattice_coordinates_round(name, shape):
    omap = new_map(name, shape)
    lat = ray_lattice(omap)
    _, e = rays.mixed_rays(lat, 4097, seed=4)
    inside, outside = eyes_of(lat)
    constants = rays.log_odds_constants()
    want_l, want_seen, marks = np.zeros(shape, np.float32), np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for eye, ends, max_range in ((inside, e[0::2], math.inf), (outside, e[1::2], 40 * RES[name])):
        omap.integrate(tensor(eye), tensor(ends), max_range=max_range)
        rays.update(rays.mark(lat, eye, ends, max_range, marks=marks), want_l, want_seen, *constants)
    got_l, got_seen = omap.log_odds.cpu().numpy(), omap.observed.cpu().numpy()
    assert np.array_equal(bits(got_l), bits(want_l)), int((bits(got_l) != bits(want_l)).sum())
    assert np.array_equal(got_seen, want_seen.astype(bool)) and got_seen.any() and (name != "fine" or not got_seen.all())
    assert (want_l > 0).any() and (want_l < 0).any()


def test_the_kernels_walk_stays_on_the_segment():
    """tests/volume_truth.py's condition, which the restatement meets on thousands of rays without a GPU, on the kernel's own
    walk: one pv.ray_marks call per ray.  The hit voxel is among the marked cells: it holds the endpoint, so `may` holds it."""
    omap = new_map("fine", (19, 13, 37))
    lat = ray_lattice(omap)
    cells_of = lambda o, e, max_range: np.argwhere(gpu_marks(omap, o, e[None], max_range) != 0)
    walked, must = truth.check_walks(lat, *rays.generic_rays(lat, 32, 31), math.inf, cells_of)
    assert walked > 300 and must >= 0.95 * walked
    truth.check_walks(lat, *rays.mixed_rays(lat, 32, 32), 40 * RES["fine"], cells_of)


@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_marks_bit_for_bit_on_an_axis_of_2048_voxels_with_walks_that_spend_the_budget(shape):
    axis = int(np.argmax(shape))
    omap = new_map("limit", shape)
    lat = ray_lattice(omap)
    long_o, long_e = rays.axis_rays(lat, axis)
    mixed_o, mixed_e = rays.mixed_rays(lat, 257, seed=5)
    lengths = [len(rays.walk(lat, o, e)) for o, e in zip(long_o, long_e)]
    assert 2048 <= max(lengths) <= sum(shape) and min(lengths) >= 2048
    o, e = np.concatenate((mixed_o, long_o)), np.concatenate((mixed_e, long_e))
    for max_range in (math.inf, 40 * RES["limit"]):
        got, want = gpu_marks(omap, o, e, max_range), rays.mark(lat, o, e, max_range)
        assert np.array_equal(got, want), (max_range, int((got != want).sum()))
    want = rays.mark(lat, long_o, long_e)  # the long rays alone: not hidden under the others
    assert np.array_equal(gpu_marks(omap, long_o, long_e, math.inf), want)
    along = np.moveaxis(want, axis, 0)
    assert along[0].any() and along[2047].any() and (along != 0).any(axis=(1, 2)).all()


# ---------------------------------------------------------------- TSDF
class Fused:
    """A volume that has integrated the wall frames on one lattice, with the restatement's state and branch counts."""

    def __init__(self, name, shape, K=3, axis=None):
        self.res = RES[name]
        self.volume = pv.TSDFVolume(self.res, ranges_of(name, shape), truncation=3 * self.res, device="cuda", max_weight=math.inf)
        assert self.volume.shape == shape
        self.truncation = self.volume.truncation
        depth, poses = tsdf_ref.wall_frames(ranges_of(name, shape), self.res, K=K, axis=axis)
        self.volume.integrate(tensor(depth), INTRINSICS, tensor(poses).cuda(), max_depth=MAX_DEPTH)
        self.state = np.zeros(shape + (2,), np.float32)
        self.hits = tsdf_ref.integrate(tsdf_ref.lattice_of(self.volume._grid.voxels._grid_desc()), self.state, depth,
                                       tsdf_ref.invert(poses), INTRINSICS, self.truncation, max_depth=MAX_DEPTH)


@functools.lru_cache(maxsize=None)
def fused(name, shape):
    return Fused(name, shape)


def fused_centres_differ(lat):
    """At how many coordinates fmaf(i, fres, fmin) is not fmin + i * fres with the product rounded first (float64 holds the
    unrounded sum): what a contracted voxel centre would change.  On the far lattice a product's rounding is a 250th of the
    sum's, so one coordinate in 131 differs; there it is the camera transform whose every product and sum rounds."""
    count = 0
    for k in range(3):
        i = np.arange(lat.shape[k])
        two_roundings = np.float32(lat.fmin[k]) + i.astype(np.float32) * np.float32(lat.fres[k])
        count += int((two_roundings != (float(lat.fmin[k]) + i * float(lat.fres[k])).astype(np.float32)).sum())
    return count


def assert_same_state(fusion):
    got = fusion.volume._state.cpu().numpy()
    assert got.shape == fusion.state.shape and np.array_equal(bits(got), bits(fusion.state)), int((bits(got) != bits(fusion.state)).sum())


@pytest.mark.parametrize("name, shape", TSDF_LATTICES)
def test_tsdf_state_bit_for_bit_where_voxel_centres_round(name, shape):
    fusion = fused(name, shape)
    for branch in ("updated", "outside", "no_return", "behind_band", "behind", "too_far"):
        assert fusion.hits[branch] > 0, branch  # the restatement really takes the branch
    assert_same_state(fusion)
    F, weight = fusion.state[..., 0], fusion.state[..., 1]
    assert 0 < (weight == 0).sum() < weight.size and (weight > 1).any()
    assert (F == 1.0).any() and (np.abs(F) < 1.0).any() and (F < 0).any()
    assert name != "fine" or fused_centres_differ(tsdf_ref.lattice_of(fusion.volume._grid.voxels._grid_desc())) > 0


@pytest.mark.parametrize("unknown", ["free", "occupied"])
@pytest.mark.parametrize("name, shape", TSDF_LATTICES)
def test_tsdf_records_and_far_field_bit_for_bit_where_voxel_centres_round(name, shape, unknown):
    fusion = fused(name, shape)
    res, trunc = fusion.res, fusion.truncation
    truncated = tsdf_ref.records(fusion.state, res, trunc, unknown_tsdf=1.0 if unknown == "free" else -1.0)
    got = pv.TSDFField(fusion.volume, unknown=unknown)._records.cpu().numpy()
    assert got.shape == truncated.shape and np.array_equal(bits(got), bits(truncated)), int((bits(got) != bits(truncated)).sum())
    length = np.linalg.norm(truncated[:, 1:].astype(np.float64), axis=1)
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all() and (length == 0).any() and (length > 0).sum() > 100
    want, sites, _ = redist.redistance(truncated.reshape(shape + (4,)), res, trunc, 3.5 * res)
    far = pv.TSDFField(fusion.volume, unknown=unknown, far_field=True, max_distance=3.5 * res)._records.cpu().numpy()
    assert np.array_equal(bits(far), bits(want)), int((bits(far) != bits(want)).sum())
    assert (sites == redist.KEPT).sum() > 100 and (sites >= 0).sum() > 100 and (sites == -1).sum() > 100


@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_tsdf_bit_for_bit_on_an_axis_of_2048_voxels(shape):
    axis = int(np.argmax(shape))
    fusion = Fused("limit", shape, K=2, axis=axis)
    assert_same_state(fusion)
    assert fusion.hits["updated"] > 2048 and fusion.hits["behind_band"] > 0 and fusion.hits["no_return"] > 0
    assert fused_centres_differ(tsdf_ref.lattice_of(fusion.volume._grid.voxels._grid_desc())) > 100
    weight = np.moveaxis(fusion.state[..., 1], axis, 0)
    assert (weight[2047] > 0).any() and (weight[0] > 0).any() and (weight == 1).any() and (weight == 2).any()
    # the records of the voxels both cameras saw, among voxels that count as unknown: differences across the 2048-long planes
    truncated = tsdf_ref.records(fusion.state, fusion.res, fusion.truncation, min_weight=1.0, unknown_tsdf=-1.0)
    got = pv.TSDFField(fusion.volume, unknown="occupied", min_weight=1.0)._records.cpu().numpy()
    assert np.array_equal(bits(got), bits(truncated)), int((bits(got) != bits(truncated)).sum())


# ---------------------------------------------------------------- redistancing
def run(rec, resolution, band=0.0, max_distance=math.inf):
    """pv.redistance on (nx, ny, nz, 4) float32 records as flat numpy arrays: (records (n, 4), sites (n,), squared (n,))."""
    values, gradients = tensor(rec[..., 0]), tensor(rec[..., 1:])
    res = pv.redistance(values, resolution=resolution, band=band, gradients=gradients if band > 0 else None, max_distance=max_distance)
    records = torch.cat((res.values[..., None], res.gradients), dim=-1).reshape(-1, 4)
    return records.cpu().numpy(), res.sites.reshape(-1).cpu().numpy(), res.squared.reshape(-1).cpu().numpy()


def assert_same(got, want):
    for what, g, w in zip(("records", "sites", "squared"), got, want):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (what, int((bits(g) != bits(w)).sum()))


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("resolution", redist.ROUNDING_RESOLUTIONS)
@pytest.mark.parametrize("field", ["smooth", "tie", "half"])
def test_redistance_bit_for_bit_where_resolution_and_range_round(field, resolution, limited):
    """max_distance = 3.5 * resolution as Python floats: Rv is not exactly 3.5 under every resolution, and on the half field
    the voxels at exactly 3.5 voxels keep their site or lose it by that (tests/test_volume_lattices.py asserts both happen)."""
    rec = redist.FIELDS[field]((19, 13, 37))
    max_distance = 3.5 * resolution if limited else math.inf
    for band in sorted({BANDS[field], 0.0}, reverse=True):
        want = redist.redistance(rec, resolution, band, max_distance)
        assert_same(run(rec, resolution, band, max_distance), want)
    sites = want[1]  # of band = 0
    assert (sites >= 0).sum() > 500 and (not limited or field == "smooth" or (sites == -1).sum() > 500)


def test_redistance_bit_for_bit_with_denormal_and_zero_samples():
    rec, replaced = redist.tiny_field((19, 13, 37))
    assert 40 < replaced.sum() < 200
    for band in (0.0, BANDS["smooth"]):
        want = redist.redistance(rec, 0.013, band)
        assert_same(run(rec, 0.013, band), want)
        sites = want[1][want[1] >= 0]
        lower, axis = np.unravel_index(sites >> 2, replaced.shape), sites & 3
        upper = tuple(lower[k] + (axis == k) for k in range(3))
        assert (replaced[lower] | replaced[upper]).any()  # winning edges with a tiny sample at one end
    assert (want[1] == redist.KEPT)[replaced.reshape(-1)].all()  # inside any band


@pytest.mark.parametrize("far", [True, False])
@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_redistance_carries_coordinate_2047_through_every_pass(shape, far):
    """One negative voxel, at the far corner or at voxel (0, 0, 0): every voxel's site is one of the three edges that leave it,
    so the packed coordinate of every line state is 2046 or 2047 (or 0), and the scans run the whole line."""
    axis = int(np.argmax(shape))
    rec = redist.one_negative_field(shape, far)
    want = redist.redistance(rec, RES["limit"])
    assert_same(run(rec, RES["limit"]), want)
    _, sites, squared = want
    assert (sites >= 0).all() and (np.bincount(sites & 3, minlength=3) > 0).all()
    lower = np.stack(np.unravel_index(sites >> 2, shape), axis=1)
    assert np.isin(lower[:, axis], (2046, 2047) if far else (0,)).all()
    opposite = np.moveaxis(squared.reshape(shape), axis, 0)[0 if far else 2047]
    assert (opposite > 2046.0 ** 2).all()


@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_redistance_of_a_smooth_field_on_an_axis_of_2048_voxels(shape):
    rec = redist.smooth_field(shape)
    for band in (0.0, BANDS["smooth"]):
        want = redist.redistance(rec, RES["limit"], band, 6 * RES["limit"])
        assert_same(run(rec, RES["limit"], band, 6 * RES["limit"]), want)
    lower = np.unravel_index(want[1][want[1] >= 0] >> 2, shape)[int(np.argmax(shape))]
    assert lower.min() < 8 and lower.max() > 2039 and (want[1] == redist.KEPT).any()  # sites at both ends of the long axis
