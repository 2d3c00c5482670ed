"""-m gpu: redistancing on the device, bit for bit against the C restatement of the contract (tests/redistance_ref.c), through
pv.redistance and TSDFVolume.to_sdf(far_field=True), and the leaf it makes in front of ray_cast and hinge_over_points."""
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import helpers as H
from tests import redistance_ref as ref
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

RES = 0.5
BANDS = {"smooth": 0.4, "tie": 25.0}  # each keeps some voxels of its field and not all (the tie field is integer valued)
BIG = (96, 80, 72)
assert BIG[0] * BIG[1] * BIG[2] > H.STREAM_GRID_ITEMS


def run(rec, resolution=RES, band=0.0, max_distance=math.inf):
    """pv.redistance on (nx, ny, nz, 4) float32 records as flat numpy arrays: (records (n, 4), sites (n,), squared (n,))."""
    values, gradients = torch.from_numpy(np.array(rec[..., 0])), torch.from_numpy(np.array(rec[..., 1:]))
    res = pv.redistance(values, resolution=resolution, band=band, gradients=gradients if band > 0 else None,
                        max_distance=max_distance)
    shape = rec.shape[:3]
    assert isinstance(res, pv.Redistance) and all(t.is_cuda and not t.requires_grad for t in res)
    assert res.values.shape == shape and res.gradients.shape == shape + (3,) and res.sites.shape == shape
    assert res.squared.shape == shape and res.sites.dtype == torch.int32 and res.squared.dtype == torch.float32
    records = torch.cat((res.values[..., None], res.gradients), dim=-1).reshape(-1, 4)
    return records.cpu().numpy(), res.sites.reshape(-1).cpu().numpy(), res.squared.reshape(-1).cpu().numpy()


def assert_same(got, want):
    for name, g, w in zip(("records", "sites", "squared"), got, want):
        assert g.shape == w.shape and np.array_equal(ref.bits(g), ref.bits(w)), (name, int((ref.bits(g) != ref.bits(w)).sum()))


@pytest.mark.parametrize("voxels", [math.inf, 3.5])
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("field", ["smooth", "tie"])
@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 3, 131), (19, 13, 37)])  # (5, 3, 131): a z line spans waves, a wave lines
def test_records_sites_and_squared_bit_for_bit(shape, field, banded, voxels):
    rec = ref.FIELDS[field](shape)
    band, max_distance = BANDS[field] if banded else 0.0, voxels * RES
    want = ref.redistance(rec, RES, band, max_distance)
    assert_same(run(rec, RES, band, max_distance), want)
    sites = want[1]
    if field == "tie" and voxels == 3.5 and shape != (2, 2, 2):
        assert 1000 < (sites == -1).sum() < sites.size - 100  # the range limit cuts: most of the lattice is further than 3.5 voxels
    else:
        assert not (sites == -1).any()
    if shape == (19, 13, 37):
        assert (np.bincount(sites[sites >= 0] & 3, minlength=3) > 300).all()  # every family wins somewhere
        assert (200 < (sites == ref.KEPT).sum() < sites.size // 2) if banded else not (sites == ref.KEPT).any()


@functools.lru_cache(maxsize=1)
def big():
    """(records, restatement's result) on the lattice past the streaming cap, worked out once."""
    rec = ref.smooth_field(BIG)
    return rec, ref.redistance(rec, RES, BANDS["smooth"], 6.0 * RES)


def test_past_the_streaming_cap_bit_for_bit():
    rec, want = big()
    assert_same(run(rec, RES, BANDS["smooth"], 6.0 * RES), want)
    tail = want[1][H.STREAM_GRID_ITEMS:]
    assert (tail >= 0).any() and (tail == ref.KEPT).any()  # the lanes' second turn redistances and keeps


def test_a_replayed_graph_gives_the_eager_bits_and_the_input_is_never_written():
    rec, want = big()
    nx, ny, nz = BIG
    n = nx * ny * nz
    records = torch.from_numpy(np.array(rec)).cuda().reshape(n, 4)
    before = records.clone()
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    sites = torch.zeros((n,), dtype=torch.int32, device="cuda")
    squared = torch.zeros((n,), dtype=torch.float32, device="cuda")
    scratch = _lib.scratch_buffer(_lib.redistance_scratch_bytes(nx, ny, nz), records.device)
    assert scratch.numel() == 36 * n

    def call():
        _lib.check(_lib.load().pvamd_redistance(_lib.ptr(records), nx, ny, nz, RES, BANDS["smooth"], 6.0 * RES, _lib.ptr(out),
                                                _lib.ptr(sites), _lib.ptr(squared), _lib.ptr(scratch), _lib.stream_ptr()),
                   "pvamd_redistance")

    call()  # warm: the library is loaded before the capture
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), sites.cpu().numpy(), squared.cpu().numpy()), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in (out, sites, squared, scratch):
        t.zero_()  # what the capture itself ran, if anything, is forgotten
    g.replay()
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), sites.cpu().numpy(), squared.cpu().numpy()), want)
    assert torch.equal(records.view(torch.int32), before.view(torch.int32))
    # sites and squared are optional
    out.zero_()
    _lib.check(_lib.load().pvamd_redistance(_lib.ptr(records), nx, ny, nz, RES, BANDS["smooth"], 6.0 * RES, _lib.ptr(out), None, None,
                                            _lib.ptr(scratch), _lib.stream_ptr()), "pvamd_redistance")
    torch.cuda.synchronize()
    assert np.array_equal(ref.bits(out.cpu().numpy()), ref.bits(want[0]))


@pytest.mark.parametrize("max_distance", [math.inf, 1.25])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_field_without_crossings(sign, max_distance):
    rec = ref.as_records(np.full((5, 3, 131), 2.0 * sign, np.float32))
    got = run(rec, max_distance=max_distance)
    assert_same(got, ref.redistance(rec, RES, 0.0, max_distance))
    assert (got[1] == -1).all() and np.isinf(got[2]).all() and (got[0][:, 0] == sign * max_distance).all() and not got[0][:, 1:].any()


def test_a_field_with_nan_and_infinite_samples():
    shape = (19, 13, 37)
    rec = ref.smooth_field(shape).copy()
    kind = np.random.default_rng(1).integers(0, 12, size=shape)
    for code, bad in enumerate((np.nan, np.inf, -np.inf)):
        rec[..., 0][kind == code] = bad
    for band, max_distance in ((0.0, math.inf), (BANDS["smooth"], 3.5 * RES)):
        want = ref.redistance(rec, RES, band, max_distance)
        assert_same(run(rec, RES, band, max_distance), want)
    nan = np.isnan(rec[..., 0].reshape(-1))
    assert nan.sum() > 100 and (want[1][nan] != ref.KEPT).all() and (want[0][nan, 0] > 0).all()  # never kept, not negative
    lower, axis = np.unravel_index(want[1][want[1] >= 0] >> 2, shape), want[1][want[1] >= 0] & 3
    upper = tuple(lower[k] + (axis == k) for k in range(3))
    assert np.isfinite(rec[..., 0][lower]).all() and np.isfinite(rec[..., 0][upper]).all()


def test_argument_errors_of_the_entry_point():
    lib = _lib.load()
    E_NULL, E_SHAPE, E_ALIGN, E_MODE = (_lib.H[f"PVAMD_E_{name}"] for name in ("NULL", "SHAPE", "ALIGN", "MODE"))
    n = 5 * 3 * 131
    records = torch.ones((n * 4 + 4,), dtype=torch.float32, device="cuda")
    out = torch.zeros((n * 4 + 4,), dtype=torch.float32, device="cuda")
    sites = torch.zeros((n + 1,), dtype=torch.int32, device="cuda")
    squared = torch.zeros((n + 1,), dtype=torch.float32, device="cuda")
    assert lib.pvamd_redistance_scratch_bytes(5, 3, 131) == 36 * n
    scratch = torch.zeros((36 * n + 4,), dtype=torch.uint8, device="cuda")
    good = dict(records=_lib.ptr(records), nx=5, ny=3, nz=131, resolution=0.5, band=0.0, max_distance=math.inf, out=_lib.ptr(out),
                sites=_lib.ptr(sites), squared=_lib.ptr(squared), scratch=_lib.ptr(scratch))

    def call(**changes):
        return lib.pvamd_redistance(*{**good, **changes}.values(), _lib.stream_ptr())

    for changes in (dict(nx=1), dict(ny=0), dict(nz=2049), dict(nx=1024, ny=1024, nz=513)):
        assert call(**changes) == E_SHAPE, changes
        assert lib.pvamd_redistance_scratch_bytes(*({**good, **changes}[k] for k in ("nx", "ny", "nz"))) == 0
    assert lib.pvamd_redistance_scratch_bytes(1024, 1024, 512) == 36 * 2 ** 29
    for changes in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=math.nan), dict(resolution=math.inf),
                    dict(band=-0.5), dict(band=math.nan), dict(max_distance=0.0), dict(max_distance=-1.0),
                    dict(max_distance=math.nan)):
        assert call(**changes) == E_MODE, changes
    assert call(nx=1, resolution=0.0, records=None) == E_SHAPE and call(resolution=0.0, records=None) == E_MODE  # the order
    for name in ("records", "out", "scratch"):
        assert call(**{name: None}) == E_NULL, name
    for name, t, step in (("records", records, 2), ("out", out, 2), ("sites", sites.view(torch.uint8), 1),
                          ("squared", squared.view(torch.uint8), 2), ("scratch", scratch, 3)):
        assert call(**{name: _lib.ptr(t[step:])}) == E_ALIGN, name
    torch.cuda.synchronize()
    assert not out.any() and not sites.any() and not squared.any()  # nothing was launched
    assert call(sites=None, squared=None, band=math.inf, scratch=_lib.ptr(scratch[4:])) == 0  # scratch only 4-byte aligned
    torch.cuda.synchronize()
    assert (out[:n * 4] == 1.0).all() and not out[n * 4:].any()  # an infinite band keeps every finite record


# ---------------------------------------------------------------- the TSDF leaf
TSDF_RES, TRUNC = 0.25, 0.75
TSDF_SHAPE, TSDF_RANGE = (19, 13, 37), [(0.0, 4.5), (-1.0, 2.0), (0.0, 9.0)]  # voxel centres are exact in float32
INTRINSICS = (40.0, 36.0, 31.5, 23.5)


@functools.lru_cache(maxsize=1)
def wall():
    """A volume over TSDF_RANGE that has seen a rippled wall through its middle from two sides, and the restatement's state."""
    centre = np.array(TSDF_RANGE).mean(axis=1)
    eyes = [centre + np.array([0.5, -0.4, 5.5]), centre + np.array([-0.6, 0.3, 5.0])]
    poses = np.stack([tsdf_ref.look_at(eye, centre) for eye in eyes])
    rows, cols = np.meshgrid(np.arange(48), np.arange(64), indexing="ij")
    depth = np.stack([np.linalg.norm(eye - centre) * (1.0 + 0.1 * np.sin(0.3 * cols + k) * np.cos(0.2 * rows))
                      for k, eye in enumerate(eyes)]).astype(np.float32)
    vol = pv.TSDFVolume(TSDF_RES, TSDF_RANGE, truncation=TRUNC, device="cuda", max_weight=math.inf)
    assert vol.shape == TSDF_SHAPE
    vol.integrate(torch.from_numpy(depth), INTRINSICS, torch.from_numpy(poses))
    state = np.zeros(TSDF_SHAPE + (2,), np.float32)
    tsdf_ref.integrate(tsdf_ref.lattice_of(vol._grid.voxels._grid_desc()), state, depth, tsdf_ref.invert(poses), INTRINSICS, TRUNC)
    assert np.array_equal(ref.bits(vol._state.cpu().numpy()), ref.bits(state))
    return vol, state


@pytest.mark.parametrize("unknown, max_distance", [("free", math.inf), ("occupied", math.inf), ("free", 1.75)])
def test_the_far_field_of_a_volume_is_its_records_redistanced_with_the_truncation_as_the_band(unknown, max_distance):
    vol, state = wall()
    truncated = tsdf_ref.records(state, TSDF_RES, TRUNC, unknown_tsdf=1.0 if unknown == "free" else -1.0)
    want, sites, _ = ref.redistance(truncated.reshape(TSDF_SHAPE + (4,)), TSDF_RES, TRUNC, max_distance)
    field = pv.TSDFField(vol, unknown=unknown, far_field=True, max_distance=max_distance)
    got = field._records.cpu().numpy()
    assert np.array_equal(ref.bits(got), ref.bits(want)), int((ref.bits(got) != ref.bits(want)).sum())
    scene = vol.to_sdf("scene", unknown=unknown, far_field=True, max_distance=max_distance)
    assert torch.equal(scene._packed.view(torch.int32), field._records.view(torch.int32))  # the records, taken as they are
    kept = sites == ref.KEPT
    assert 500 < kept.sum() < kept.size - 500 and np.array_equal(ref.bits(want[kept]), ref.bits(truncated[kept]))
    assert (np.abs(want[~kept, 0]) > TRUNC).any() and (np.signbit(want[:, 0]) == np.signbit(truncated[:, 0])).all()
    assert np.array_equal(field.surface_bounding_box().numpy(), pv.TSDFField(vol, unknown=unknown).surface_bounding_box().numpy())
    # far_field=False is today's path and bits
    plain = pv.TSDFField(vol, unknown=unknown, far_field=False)
    assert np.array_equal(ref.bits(plain._records.cpu().numpy()), ref.bits(truncated))


def test_the_hinge_with_a_margin_of_twice_the_truncation_counts_what_the_truncated_leaf_cannot():
    vol, state = wall()
    truncated = tsdf_ref.records(state, TSDF_RES, TRUNC)
    want = ref.redistance(truncated.reshape(TSDF_SHAPE + (4,)), TSDF_RES, TRUNC)[0]
    inner = np.zeros(TSDF_SHAPE, bool)
    inner[1:-1, 1:-1, 1:-1] = True  # the centres of the inner voxels: each reads its own record
    centres = tsdf_ref.centres(tsdf_ref.lattice_of(vol._grid.voxels._grid_desc()))[inner]
    points = torch.from_numpy(centres).cuda()
    margin = 2 * TRUNC
    counts = {}
    for far_field in (False, True):
        comp = pv.ComposedSDF([vol.to_sdf("scene", far_field=far_field)], None)
        comp.set_transforms(torch.eye(4, device="cuda")[None], batch_dim=(1,))
        result = comp.hinge_over_points(points, margin)
        counts[far_field] = int(result.counts[0])
        values = (want if far_field else truncated)[inner.reshape(-1), 0]
        assert counts[far_field] == int((values < np.float32(margin)).sum())
        hinge = (np.clip(np.float32(margin) - values, 0, None).astype(np.float32) ** 2).astype(np.float64).sum()
        assert abs(float(result.values[0]) - hinge) <= 1e-6 * hinge
    assert counts[False] == len(centres)  # truncated: every point reads less than the margin, with no gradient to push it
    assert 0 < counts[True] < counts[False]


def test_the_leaf_in_front_of_ray_cast_steps_past_the_truncation():
    radius, res, ranges, intrinsics = 0.3, 0.02, [(-0.5, 0.5)] * 3, (150.0, 150.0, 79.5, 59.5)
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, intrinsics, 120, 160, (0.0, 0.0, 0.0), radius)
    vol = pv.TSDFVolume(res, ranges, truncation=0.06, device="cuda")
    vol.integrate(torch.from_numpy(depth), intrinsics, torch.from_numpy(poses))
    eye = np.array([0.44, 0.2, 0.1])  # inside the lattice, 0.19 from the ball: three truncations
    target = torch.nn.functional.normalize(torch.randn(500, 3, generator=torch.Generator().manual_seed(2)), dim=-1) * 0.1
    origins = torch.from_numpy(eye).float().expand(500, 3).contiguous().cuda()
    directions = torch.nn.functional.normalize(target - torch.from_numpy(eye).float(), dim=-1).cuda()  # toward the ball's core
    o, d = origins.double().cpu().numpy(), directions.double().cpu().numpy()
    b = (o * d).sum(-1)
    true = -b - np.sqrt(b * b - ((o * o).sum(-1) - radius * radius))
    casts = {}
    for far_field in (False, True):
        scene = vol.to_sdf("scene", far_field=far_field)
        casts[far_field] = cast = scene.ray_cast(origins, directions, step_scale=1.0, max_steps=64)
        assert (cast.status == pv.RAY_HIT).all()
        # a hit is declared inside the band, whose records both leaves share: within the truncation of the sphere, the bound
        # tests/test_tsdf_gpu.py sets for the truncated leaf
        assert np.abs(cast.t.cpu().numpy() - true).max() < 0.06
    first = vol.to_sdf("scene", far_field=True)(origins[:1])[0]
    assert float(first) > 2 * 0.06  # the first step alone is longer than two truncations
    # the truncated leaf reads 0.06 until it is inside the band, 0.13 away: three evaluations where the far field needs one,
    # and one evaluation of slack for where each of them enters the band
    assert float(casts[True].steps.float().mean()) <= float(casts[False].steps.float().mean()) - 1.0
