"""Ray integration without a GPU: the argument errors of OccupancyMap / ray_marks, the header constants, and the properties the
contract's statements (include/pvamd.h "Ray integration") must have, checked on their C restatement (tests/ray_integrate_ref.c)."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib, occupancy_map
from tests import ray_integrate_ref as ref

LATTICES = [(5, 7, 9), (2, 3, 300)]
RANGE = [(-1.0, 1.0), (-1.0, 1.0), (0.0, 1.5)]


# ---------------------------------------------------------------- the Python layer
def test_header_constants_reach_the_binding():
    assert _lib.MARK_FREE == _lib.H["PVAMD_MARK_FREE"] == ref.MARK_FREE == 1
    assert _lib.MARK_HIT == _lib.H["PVAMD_MARK_HIT"] == ref.MARK_HIT == 2
    for name in ("pvamd_ray_mark", "pvamd_occupancy_update"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pvamd_ray_mark"][1]) == 8 and len(_lib.SIGNATURES["pvamd_occupancy_update"][1]) == 9
    assert pv.OccupancyMap is not None and pv.ray_marks is not None
    assert _lib.LATTICE_MAX_AXIS == _lib.H["PVAMD_LATTICE_MAX_AXIS"] == occupancy_map.MAX_AXIS == 2048
    assert _lib.RAY_MARK_MIN_AXIS == _lib.H["PVAMD_RAY_MARK_MIN_AXIS"] == occupancy_map.MIN_AXIS == 2


@pytest.mark.parametrize("kwargs", [
    dict(range_per_dim=[(-1, 1), (-1, 1)]),                              # not 3-D
    dict(range_per_dim=[(-1, 1), (-1, 1), (0, 1), (0, 1)]),
    dict(range_per_dim=[(-1, 1), (-1, 1), (0, 0.004)]),                  # one voxel along z
    dict(resolution=0.001, range_per_dim=[(-1, 1.1), (-1, 1), (0, 1)]),  # 2101 voxels along x
    dict(resolution=0.0), dict(resolution=math.nan),
    dict(prob_hit=0.5), dict(prob_hit=1.0), dict(prob_hit=1.2), dict(prob_hit=math.nan),
    dict(prob_miss=0.5), dict(prob_miss=0.0), dict(prob_miss=-0.1), dict(prob_miss=0.7),
    dict(clamp=(0.0, 0.97)), dict(clamp=(0.12, 1.0)), dict(clamp=(0.5, 0.97)), dict(clamp=(0.12, 0.5)), dict(clamp=(0.97, 0.12)),
    dict(clamp=(math.nan, 0.97)),
])
def test_construction_errors_need_no_gpu(kwargs):
    args = dict(resolution=0.02, range_per_dim=RANGE, device="cuda")
    args.update(kwargs)
    with pytest.raises(ValueError):
        pv.OccupancyMap(**args)


@pytest.fixture(scope="module")
def host_map():
    """A map that lives in host memory: everything but the scan itself works there."""
    return pv.OccupancyMap(0.25, RANGE, device="cpu")


def test_the_constants_are_float64_logs_rounded_once(host_map):
    want = ref.log_odds_constants()
    got = (host_map.l_hit, host_map.l_miss, host_map.l_min, host_map.l_max)
    assert [np.float32(g) for g in got] == list(want) and all(np.float32(g) == g for g in got)
    assert host_map.shape == (9, 9, 7) and host_map.log_odds.dtype == torch.float32 and host_map.observed.dtype == torch.bool
    assert not host_map.observed.any() and not host_map.occupied().any() and host_map.occupied(unknown="occupied").all()
    assert torch.equal(host_map.probability(), torch.full((9, 9, 7), 0.5))


@pytest.mark.parametrize("call", ["integrate", "ray_marks"])
@pytest.mark.parametrize("eye, endpoints, max_range", [
    (torch.zeros(2), torch.zeros(4, 3), math.inf),           # last dimension other than 3
    (torch.zeros(3), torch.zeros(4, 2), math.inf),
    (torch.zeros(3), torch.zeros(()), math.inf),
    (torch.zeros(5, 3), torch.zeros(4, 3), math.inf),        # shapes that do not broadcast
    (torch.zeros(2, 1, 3), torch.zeros(3, 4, 3), math.inf),
    (torch.zeros(3), torch.zeros(4, 3), math.nan),           # max_range
    (torch.zeros(3), torch.zeros(4, 3), 0.0),
    (torch.zeros(3), torch.zeros(4, 3), -1.0),
])
def test_scan_errors_are_raised_before_a_gpu_is_asked_for(host_map, call, eye, endpoints, max_range):
    with pytest.raises(ValueError):
        if call == "integrate":
            host_map.integrate(eye, endpoints, max_range=max_range)
        else:
            pv.ray_marks(host_map, eye, endpoints, max_range=max_range)


def test_occupied_and_to_sdf_errors(host_map):
    with pytest.raises(ValueError):
        host_map.occupied(unknown="maybe")
    with pytest.raises(ValueError):
        host_map.to_sdf("scene", unknown="maybe")
    for threshold in ("0.5", None, 0.5j, torch.tensor(0.5), True):
        with pytest.raises(TypeError):
            host_map.occupied(threshold=threshold)
    assert not host_map.occupied(threshold=np.float32(0.5)).any()


def test_no_rays_is_a_no_op_and_a_scan_without_a_gpu_is_a_loud_error(host_map):
    host_map.integrate(torch.zeros(3), torch.zeros(0, 3))
    assert pv.ray_marks(host_map, torch.zeros(3), torch.zeros(0, 3)).shape == (9, 9, 7)
    assert not host_map.observed.any()
    with pytest.raises(_lib.PvamdError):
        host_map.integrate(torch.zeros(3), torch.ones(4, 3))


# ---------------------------------------------------------------- properties of the contract's statements
@pytest.mark.parametrize("shape", LATTICES)
def test_walks_repeat_no_cell_move_one_cell_along_one_axis_and_stay_within_the_budget(shape):
    lat = ref.unit_lattice(shape)
    for seed, rays in ((1, ref.mixed_rays(lat, 3000, 1)), (2, ref.generic_rays(lat, 3000, 2))):
        walked = 0
        for o, e in zip(*rays):
            for max_range in (np.inf, 2.5):
                cells = ref.walk(lat, o, e, max_range)
                assert len(cells) <= sum(shape)
                if len(cells) == 0:
                    continue
                walked += 1
                assert (cells >= 0).all() and (cells < np.array(shape)).all()
                assert len(np.unique(cells, axis=0)) == len(cells)
                assert (np.abs(np.diff(cells, axis=0)).sum(axis=1) == 1).all()
        assert walked > 1000, (seed, walked)


@pytest.mark.parametrize("shape", LATTICES)
def test_an_axis_parallel_ray_through_voxel_centres_marks_exactly_the_cells_between_its_ends(shape):
    lat = ref.unit_lattice(shape)
    for axis in range(3):
        for lo, hi in ((0, shape[axis] - 1), (1, shape[axis] - 1), (0, 0), (shape[axis] - 1, 0)):
            o, e = np.array([1.0, 1.0, 1.0], np.float32), np.array([1.0, 1.0, 1.0], np.float32)
            o[axis], e[axis] = lo, hi
            marks = ref.mark(lat, o, e[None])
            want = np.zeros(shape, np.uint8)
            index = [1, 1, 1]
            for i in range(min(lo, hi), max(lo, hi) + 1):
                index[axis] = i
                want[tuple(index)] = ref.MARK_FREE
            index[axis] = hi
            want[tuple(index)] = ref.MARK_HIT
            assert np.array_equal(marks, want), (axis, lo, hi)


@pytest.mark.parametrize("shape", LATTICES)
def test_zero_length_outside_and_non_finite_rays(shape):
    lat = ref.unit_lattice(shape)
    p = np.array([0.75, 1.25, shape[2] - 1.4], np.float32)
    marks = ref.mark(lat, p, p[None])
    assert marks.sum() == ref.MARK_HIT and marks[1, 1, shape[2] - 1] == ref.MARK_HIT  # a lone HIT
    n = np.array(shape, np.float32)
    outside = [(n + 1, n + 4), (-n - 3, np.array([-1, 3, 2], np.float32)), (np.array([-2, 1, 1], np.float32), np.array([-0.6, 1, 1], np.float32)),
               (np.array([1, 1, -5], np.float32), np.array([1, n[1] + 5, -1], np.float32))]
    for o, e in outside:
        assert not ref.mark(lat, np.asarray(o, np.float32), np.asarray(e, np.float32)[None]).any(), (o, e)
    for bad in (np.nan, np.inf, -np.inf):
        for end in range(2):
            for k in range(3):
                ray = [np.array([0.2, 0.3, 0.4], np.float32), np.array([1.2, 1.3, 1.4], np.float32)]
                ray[end][k] = bad
                assert not ref.mark(lat, ray[0], ray[1][None]).any(), (bad, end, k)
                assert len(ref.walk(lat, ray[0], ray[1])) == 0


@pytest.mark.parametrize("shape", LATTICES)
def test_a_ray_beyond_max_range_has_no_hit_and_carves_no_farther(shape):
    lat = ref.unit_lattice(shape)
    origins, endpoints = ref.generic_rays(lat, 2000, 5)
    max_range = 2.5
    diagonal = math.sqrt(3.0)
    cut = 0
    for o, e in zip(origins, endpoints):
        length = np.linalg.norm(e.astype(np.float64) - o.astype(np.float64))
        marks = ref.mark(lat, o, e[None], max_range)
        if length > max_range + 1e-3:
            cut += 1
            assert not (marks == ref.MARK_HIT).any()
        elif length < max_range - 1e-3:
            assert (marks == ref.MARK_HIT).sum() == 1
        touched = np.argwhere(marks != 0)
        if len(touched):
            assert np.linalg.norm(touched - o.astype(np.float64), axis=1).max() <= max_range + diagonal
    assert cut > 300


@pytest.mark.parametrize("shape", LATTICES)
def test_permuting_the_rays_leaves_the_marks_unchanged(shape):
    lat = ref.unit_lattice(shape)
    o, e = ref.mixed_rays(lat, 4097, 7)
    for max_range in (np.inf, 3.0):
        marks = ref.mark(lat, o, e, max_range)
        assert {ref.MARK_FREE, ref.MARK_HIT} <= set(np.unique(marks))
        for seed in (1, 2):
            order = np.random.default_rng(seed).permutation(len(o))
            assert np.array_equal(ref.mark(lat, o[order], e[order], max_range), marks)
        halves = ref.mark(lat, o[:2000], e[:2000], max_range)  # and marks of two calls accumulate to the same scan
        assert np.array_equal(ref.mark(lat, o[2000:], e[2000:], max_range, marks=halves), marks)


@pytest.mark.parametrize("shape", LATTICES)
def test_walks_end_in_the_endpoints_voxel(shape):
    """The two conditions on the contract: a generic ray that ends inside the grid ends its walk in the endpoint's voxel (at least
    99 % of them), and a ray between half-integer lattice coordinates ends within one cell per axis of it (always)."""
    lat = ref.unit_lattice(shape)
    origins, endpoints = ref.generic_rays(lat, 10_000, 11)
    ends = 0
    for o, e in zip(origins, endpoints):
        cells = ref.walk(lat, o, e)
        assert len(cells)
        ends += np.array_equal(cells[-1], np.rint(e.astype(np.float64)))
    assert ends >= 0.99 * len(origins), ends
    rng = np.random.default_rng(12)
    n = np.array(shape)
    snapped_o = (np.floor(rng.uniform(-3.5, n + 2.5, size=(5000, 3))) + 0.5).astype(np.float32)
    snapped_e = (np.floor(rng.uniform(0, n - 1, size=(5000, 3))) + 0.5).astype(np.float32)  # 0.5 .. n - 1.5: in range, on cell corners
    for o, e in zip(snapped_o, snapped_e):
        cells = ref.walk(lat, o, e)
        assert len(cells), (o, e)
        marks = ref.mark(lat, o, e[None])
        hit = np.argwhere(marks == ref.MARK_HIT)
        assert len(hit) == 1
        assert np.abs(cells[-1] - hit[0]).max() <= 1, (o, e, cells[-1], hit[0])
