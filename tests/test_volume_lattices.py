"""The volume pipeline's restatements (tests/ray_integrate_ref.c, tests/tsdf_ref.c, tests/redistance_ref.c) against float64
references (tests/volume_truth.py) and brute force, without a GPU, on the lattices of tests/test_volume_lattices_gpu.py: a fine
one that rounds, one far from the origin, and axes at PVAMD_LATTICE_MAX_AXIS.  The GPU file ties the kernels to the restatements
bit for bit; this file ties the restatements to the geometry.  Measured figures: profiles/volume_lattice_tests.md."""
import numpy as np
import pytest

from tests import ray_integrate_ref as rays
from tests import redistance_ref as redist
from tests import tsdf_ref
from tests import volume_truth as truth

# (shape, low, resolution): the lattices of the GPU file, without the library
FINE = ((19, 13, 37), (3.37, -1.21, 0.113), 0.013)
FAR = ((5, 7, 9), (1000.37, -998.21, 500.113), 0.02)
LIMIT_Z = ((3, 2, 2048), (3.37, -1.21, -20.0), 0.02)
LIMIT_SHAPES = [(2048, 2, 3), (2, 2048, 3), (3, 2, 2048)]
EPS = 1e-3  # voxels: float32 lattice coordinates up to 2051 carry about three roundings of 2^-24 relative each, some 4e-4


# ---------------------------------------------------------------- the walk against the segment itself
@pytest.mark.parametrize("shape, low, res", [FINE, FAR, LIMIT_Z], ids=["fine", "far", "limit-z"])
def test_a_walk_visits_every_cell_the_segment_crosses_and_no_cell_it_misses(shape, low, res):
    """must <= walked <= may for every ray, none left out.  Measured here: no cell missed and none extra; `must` holds 99.5 %
    of the cells walked on the generic rays of each lattice."""
    lat = rays.unit_lattice(shape, low, res)
    cells_of = lambda o, e, max_range: rays.walk(lat, o, e, max_range)
    generic = rays.generic_rays(lat, 1000, 21)
    walked = must = 0
    for max_range in (np.inf, 40 * res):
        w, m = truth.check_walks(lat, *generic, max_range, cells_of, EPS)
        walked, must = walked + w, must + m
        truth.check_walks(lat, *rays.mixed_rays(lat, 1000, 22), max_range, cells_of, EPS)
    print(f"{shape}: must holds {must} of the {walked} cells walked on generic rays, {must / walked:.4f}")
    assert walked > 5000 and must >= 0.95 * walked  # the lower bound is nearly the walk: the check is not vacuous


def test_the_walk_bounds_of_an_axis_parallel_ray_are_its_cells():
    lat = rays.unit_lattice((5, 7, 9), FINE[1], FINE[2])
    o, e = rays.world(lat, [1.0, 2.25, -3.0]), rays.world(lat, [1.0, 2.25, 4.25])
    must, may = truth.walk_bounds(lat, o, e)
    want = np.zeros((5, 7, 9), bool)
    want[1, 2, 0:5] = True
    assert np.array_equal(must, want) and np.array_equal(may, want)
    must, may = truth.walk_bounds(lat, o, e, max_range=5.0 * FINE[2])  # cut at z = 2.0 in lattice coordinates
    assert must[1, 2, :2].all() and not must[1, 2, 3:].any() and may[1, 2, 2] and not may[1, 2, 3:].any()
    must, may = truth.walk_bounds(lat, o, o)  # a point outside: nothing
    assert not must.any() and not may.any()


# ---------------------------------------------------------------- the TSDF restatement against float64
# |F - F64| of the decided voxels, F in units of the truncation: 4 x the worst difference of the restatement measured on FINE and
# on the (19, 13, 37) lattice of tests/test_tsdf_gpu.py (profiles/volume_lattice_tests.md, measured on the CPU)
TSDF_BOUND = 4 * 1.01e-5
UNDECIDED_CAP = 0.05
INTRINSICS = (40.0, 36.0, 31.5, 23.5)
MAX_DEPTH = 500.0


def tsdf_against_float64(shape, low, res):
    """(|F - F64| over the decided voxels, weights equal there, undecided share of the float64 reference's updates, hits)."""
    lat = tsdf_ref.make_lattice(shape, low, res)
    ranges = [(lo, lo + (n - 1) * res) for lo, n in zip(low, shape)]
    depth, poses = tsdf_ref.wall_frames(ranges, res)
    inverse = tsdf_ref.invert(poses)
    state = np.zeros(shape + (2,), np.float32)
    hits = tsdf_ref.integrate(lat, state, depth, inverse, INTRINSICS, 3 * res, max_depth=MAX_DEPTH)
    want, updated, undecided = truth.tsdf_integrate64(lat, depth, inverse, INTRINSICS, 3 * res, max_depth=MAX_DEPTH,
                                                      length_tol=1e-3 * res)
    decided = ~undecided
    difference = np.abs(state[..., 0].astype(np.float64) - want[..., 0])[decided]
    return difference, state[..., 1][decided] == want[..., 1][decided], undecided.sum() / updated.sum(), hits, updated


def test_the_tsdf_restatement_is_the_float64_statements_on_a_lattice_that_rounds():
    """Measured here: worst |F - F64| 1.009e-05 over the decided voxels, 211 undecided voxels against 6353 updated ones (3.3 %:
    cx = 31.5 puts the optical axis, which the first camera points at the middle voxel, on a pixel boundary)."""
    difference, same_weight, share, hits, updated = tsdf_against_float64(*FINE)
    print(f"worst |F - F64| {difference.max():.3e}, undecided {share:.4f} of {updated.sum()} updated voxels")
    for branch in ("updated", "outside", "no_return", "behind_band", "behind", "too_far"):
        assert hits[branch] > 0, branch
    assert updated.sum() > 2000
    assert share <= UNDECIDED_CAP
    assert same_weight.all(), int((~same_weight).sum())  # decided: updated by the same frames, or by none
    assert difference.max() <= TSDF_BOUND


# ---------------------------------------------------------------- the range limit where max_distance / resolution rounds
def test_a_voxel_at_exactly_the_range_limit_keeps_its_site_under_one_resolution_and_loses_it_under_another():
    """max_distance = 3.5 * resolution as Python floats, both rounded to float32 by the call: Rv = max_distance / resolution is
    3.4999998 under 0.013 and 3.5 under 0.02 and 0.037.  The tie field of this shape has no voxel at squared == 12.25 (none of its
    crossings sits at f = 0.5), so it cannot show the difference; the half field has two slabs of them."""
    shape = (19, 13, 37)
    assert not (redist.redistance(redist.tie_field(shape))[2] == 12.25).any()
    rec = redist.half_field(shape)
    at_limit = redist.redistance(rec)[2] == 12.25
    assert at_limit.sum() == 2 * 13 * 37
    outcomes = set()
    for resolution in redist.ROUNDING_RESOLUTIONS:
        _, sites, squared = redist.redistance(rec, resolution, 0.0, 3.5 * resolution)
        kept = sites[at_limit] >= 0
        assert kept.all() or not kept.any()
        assert (squared[at_limit] == (12.25 if kept.all() else np.inf)).all()
        outcomes.add(bool(kept.all()))
        assert (sites[~at_limit & (redist.redistance(rec)[2] < 12.25)] >= 0).all()
    assert outcomes == {True, False}


# ---------------------------------------------------------------- the nested form against brute force on the new shapes
def field(name, shape):
    if name == "tiny":
        return redist.tiny_field(shape)[0]
    return redist.one_negative_field(shape, far=name == "far")


@pytest.mark.parametrize("name, shape", [(name, shape) for shape in LIMIT_SHAPES for name in ("far", "near")] + [("tiny", (19, 13, 37))])
def test_the_nested_form_is_the_minimum_over_all_crossings_on_the_limit_shapes_and_the_tiny_samples(name, shape):
    rec = field(name, shape)
    out, sites, squared = redist.redistance(rec)
    want = redist.brute(rec)
    assert np.isfinite(want).all()
    assert np.array_equal(redist.bits(squared), redist.bits(want)), int((redist.bits(squared) != redist.bits(want)).sum())
    assert (sites >= 0).all() and np.array_equal(redist.bits(redist.site_costs(rec, sites)), redist.bits(squared))
    values = rec[..., 0].reshape(-1)
    assert np.array_equal(out[:, 0], np.where(values < 0, -np.sqrt(squared), np.sqrt(squared)))
    length = np.linalg.norm(out[:, 1:].astype(np.float64), axis=1)
    assert (np.abs(length[squared > 0] - 1) < 1e-6).all() and not out[squared == 0, 1:].any()
    if name == "tiny":
        assert (np.bincount(sites & 3, minlength=3) > 0).all()
    else:
        long_axis = int(np.argmax(shape))
        lower = np.stack(np.unravel_index(sites >> 2, shape), axis=1)
        assert np.isin(lower[:, long_axis], (2046, 2047) if name == "far" else (0,)).all()
        assert squared.max() > 2046.0 ** 2
