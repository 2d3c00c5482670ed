"""TSDF fusion without a GPU: the argument errors of TSDFVolume / TSDFField, the binding, and the properties the contract's
statements (include/pvamd.h "TSDF integration") must have, checked on their C restatement (tests/tsdf_ref.c)."""
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import tsdf as tsdf_module
from tests import tsdf_ref as ref

RANGE = [(-1.0, 1.0), (-1.0, 1.0), (0.0, 1.5)]
INTRINSICS = (150.0, 150.0, 79.5, 59.5)


# ---------------------------------------------------------------- the Python layer
def test_the_entry_points_reach_the_binding():
    assert len(_lib.SIGNATURES["pvamd_tsdf_integrate"][1]) == 16 and len(_lib.SIGNATURES["pvamd_tsdf_records"][1]) == 10
    assert _lib.ABI_VERSION == 16
    assert pv.TSDFVolume is tsdf_module.TSDFVolume and pv.TSDFField is tsdf_module.TSDFField
    assert issubclass(pv.TSDFField, pv.OccupancySDF)  # what CachedSDF takes records from as they are
    # the lattice limits: defined in the header, read by the binding, used by the module and, below, by the library
    MIN, MAX = tsdf_module.MIN_AXIS, tsdf_module.MAX_AXIS
    assert _lib.LATTICE_MAX_AXIS == _lib.H["PVAMD_LATTICE_MAX_AXIS"] == MAX == 2048
    assert _lib.TSDF_MIN_AXIS == _lib.H["PVAMD_TSDF_MIN_AXIS"] == MIN == 2
    assert _lib.TSDF_MAX_VOXELS == _lib.H["PVAMD_TSDF_MAX_VOXELS"] == 2 ** 31 - 1
    assert _lib.TSDF_MAX_PIXELS == _lib.H["PVAMD_TSDF_MAX_PIXELS"] == tsdf_module.MAX_PIXELS == 2 ** 31 - 1
    lib = _lib.load()
    for axis in range(3):
        for n, want in ((MAX + 1, _lib.E_SHAPE), (MIN - 1, _lib.E_SHAPE), (MAX, _lib.H["PVAMD_E_NULL"])):
            shape = [MIN] * 3  # the shape is tested before the pointers: no GPU is touched
            shape[axis] = n
            assert lib.pvamd_tsdf_records(None, *shape, 0.02, 0.06, 0.0, 1.0, None, None) == want, shape
    assert lib.pvamd_tsdf_records(None, MAX, MAX, MAX, 0.02, 0.06, 0.0, 1.0, None, None) == _lib.E_SHAPE  # too many voxels


@pytest.mark.parametrize("kwargs", [
    dict(range_per_dim=[(-1, 1), (-1, 1)]),                              # not 3-D
    dict(range_per_dim=[(-1, 1), (-1, 1), (0, 1), (0, 1)]),
    dict(range_per_dim=[(-1, 1), (-1, 1), (0, 0.004)]),                  # one voxel along z
    dict(resolution=0.001, range_per_dim=[(-1, 1.1), (-1, 1), (0, 1)]),  # 2101 voxels along x
    dict(resolution=0.0), dict(resolution=-0.02), dict(resolution=math.nan), dict(resolution=math.inf),
    dict(truncation=0.0), dict(truncation=-0.06), dict(truncation=math.nan), dict(truncation=math.inf),
    dict(max_weight=0.0), dict(max_weight=-1.0), dict(max_weight=math.nan),
])
def test_construction_errors_need_no_gpu(kwargs, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    args = dict(resolution=0.02, range_per_dim=RANGE, truncation=0.06, device="cuda")
    args.update(kwargs)
    with pytest.raises(ValueError):
        pv.TSDFVolume(**args)


@pytest.fixture(scope="module")
def host_volume():
    """A volume that lives in host memory: everything but the kernels works there."""
    return pv.TSDFVolume(0.25, RANGE, truncation=0.75, device="cpu", max_weight=math.inf)


def test_a_fresh_volume(host_volume):
    assert host_volume.shape == (9, 9, 7) and host_volume.max_weight == math.inf
    assert host_volume.tsdf.shape == host_volume.weight.shape == (9, 9, 7)
    assert host_volume.tsdf.dtype == host_volume.weight.dtype == torch.float32
    assert host_volume.tsdf.data_ptr() == host_volume._state.data_ptr()  # views of the one state tensor
    assert host_volume.weight.data_ptr() == host_volume._state.data_ptr() + 4
    assert not host_volume._state.view(torch.int32).any()
    host_volume.weight[1, 2, 3] = 2.0
    assert host_volume._state[1, 2, 3, 1] == 2.0
    host_volume.reset()
    assert not host_volume._state.view(torch.int32).any()


DEPTH, POSE = torch.ones(4, 6), torch.eye(4)


@pytest.mark.parametrize("args, kwargs", [
    ((torch.ones(6), INTRINSICS, POSE), {}),                                   # depth neither 2-D nor 3-D
    ((torch.ones(1, 1, 4, 6), INTRINSICS, POSE), {}),
    ((torch.ones(2, 4, 6), INTRINSICS, POSE), {}),                             # one pose does not broadcast over two frames
    ((torch.ones(2, 4, 6), INTRINSICS, torch.eye(4).expand(3, 4, 4)), {}),
    ((DEPTH, INTRINSICS, torch.eye(4).expand(2, 4, 4)), {}),
    ((DEPTH, INTRINSICS, torch.eye(3)), {}),                                   # not a pose
    ((torch.ones(1, 1, 1).expand(2, 2 ** 15, 2 ** 15), INTRINSICS, torch.eye(4).expand(2, 4, 4)), {}),  # 2^31 pixels
    ((DEPTH, (0.0, 150.0, 3.0, 2.0), POSE), {}),                               # intrinsics
    ((DEPTH, (150.0, -1.0, 3.0, 2.0), POSE), {}),
    ((DEPTH, (150.0, 150.0, math.nan, 2.0), POSE), {}),
    ((DEPTH, (150.0, 150.0, 3.0, math.inf), POSE), {}),
    ((DEPTH, (150.0, 150.0, 3.0), POSE), {}),
    ((DEPTH, torch.tensor([[0.0, 0.0, 3.0], [0.0, 150.0, 2.0], [0.0, 0.0, 1.0]]), POSE), {}),
    ((DEPTH, INTRINSICS, POSE), dict(max_depth=0.0)),
    ((DEPTH, INTRINSICS, POSE), dict(max_depth=-1.0)),
    ((DEPTH, INTRINSICS, POSE), dict(max_depth=math.nan)),
    ((DEPTH, INTRINSICS, POSE), dict(weight=0.0)),
    ((DEPTH, INTRINSICS, POSE), dict(weight=-1.0)),
    ((DEPTH, INTRINSICS, POSE), dict(weight=math.nan)),
    ((DEPTH, INTRINSICS, POSE), dict(weight=math.inf)),
])
def test_frame_errors_are_raised_before_a_gpu_is_asked_for(host_volume, args, kwargs, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    with pytest.raises(ValueError):
        host_volume.integrate(*args, **kwargs)


def test_no_frames_are_a_no_op_and_a_host_volume_has_no_kernel(host_volume):
    host_volume.integrate(torch.ones(0, 4, 6), INTRINSICS, torch.eye(4).expand(0, 4, 4))
    assert not host_volume._state.view(torch.int32).any()
    with pytest.raises(_lib.PvamdError):
        host_volume.integrate(DEPTH, INTRINSICS, POSE)
    with pytest.raises(_lib.PvamdError):
        host_volume.integrate(DEPTH.to(torch.int16), torch.tensor([[150.0, 0.0, 3.0], [0.0, 150.0, 2.0], [0.0, 0.0, 1.0]]), POSE[None],
                              max_depth=math.inf, depth_scale=0.001)
    with pytest.raises(_lib.PvamdError):
        pv.TSDFField(host_volume)
    with pytest.raises(_lib.PvamdError):
        host_volume.to_sdf("scene")


def test_field_errors_are_raised_before_a_gpu_is_asked_for(host_volume, monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a GPU was asked for before the arguments were checked"))
    for unknown in ("unknown", None, "FREE"):
        with pytest.raises(ValueError):
            pv.TSDFField(host_volume, unknown=unknown)
        with pytest.raises(ValueError):
            host_volume.to_sdf("scene", unknown=unknown)
    for min_weight in ("1", None, True, 1j):
        with pytest.raises(TypeError):
            pv.TSDFField(host_volume, min_weight=min_weight)
        with pytest.raises(TypeError):
            host_volume.to_sdf("scene", min_weight=min_weight)


def test_the_pose_inverse_is_rigid_float64_rounded_once():
    poses = np.stack([ref.look_at((0.9, -0.4, 0.3), (0.1, 0.0, 0.2)), ref.look_at((0.0, 0.1, 2.0), (0.0, 0.0, 0.0))])
    got = tsdf_module.camera_from_volume(torch.from_numpy(poses))
    assert got.dtype == torch.float32 and got.shape == (2, 3, 4)
    assert np.array_equal(got.numpy().view(np.int32), ref.invert(poses).view(np.int32))
    exact = np.linalg.inv(poses)[:, :3, :]
    assert np.abs(got.numpy() - exact).max() < 1e-6
    assert torch.equal(tsdf_module.camera_from_volume(torch.from_numpy(poses[0])), got[:1])  # (4, 4) is one frame
    assert torch.equal(tsdf_module.camera_from_volume(torch.from_numpy(poses).float().double()),
                       tsdf_module.camera_from_volume(torch.from_numpy(poses).float()))  # float32 poses: inverted in float64


# ---------------------------------------------------------------- the statements, on their restatement
BALL_RADIUS, BALL_RES, BALL_TRUNC = 0.3, 0.02, 0.06


@functools.lru_cache(maxsize=None)
def ball_scene():
    """The issue's scene: a ball of radius 0.3 at the origin on a 51^3 lattice at 0.02, six axis views of 160 x 120 at f = 150
    from one metre.  (lattice, depth, inverse poses): read-only, shared."""
    lat = ref.make_lattice((51, 51, 51), (-0.5, -0.5, -0.5), BALL_RES)
    poses = ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = ref.ball_depth(poses, INTRINSICS, 120, 160, (0.0, 0.0, 0.0), BALL_RADIUS)
    inverse = ref.invert(poses)
    depth.flags.writeable = inverse.flags.writeable = False
    return lat, depth, inverse


def fused(lat, depth, inverse, state=None, **kwargs):
    state = np.zeros(lat.dims + (2,), np.float32) if state is None else state.copy()
    hits = ref.integrate(lat, state, depth, inverse, INTRINSICS, BALL_TRUNC, **kwargs)
    return state, hits


def test_frames_in_one_call_equal_sequential_calls():
    lat, depth, inverse = ball_scene()
    for kwargs in (dict(), dict(max_weight=2.0), dict(weight=0.5, max_depth=0.8)):
        once, hits = fused(lat, depth, inverse, **kwargs)
        step = np.zeros_like(once)
        for k in range(len(depth)):
            step, _ = fused(lat, depth[k], inverse[k], state=step, **kwargs)
        assert np.array_equal(once.view(np.int32), step.view(np.int32))
        assert hits["updated"] > 10000 and hits["no_return"] > 0 and hits["outside"] > 0 and hits["behind_band"] > 0
    assert hits["too_far"] > 0
    swapped, _ = fused(lat, depth[::-1], inverse[::-1], max_weight=2.0)  # the order matters once the cap is reached
    capped, _ = fused(lat, depth, inverse, max_weight=2.0)
    assert not np.array_equal(swapped.view(np.int32), capped.view(np.int32))


def test_the_weight_cap_holds():
    lat, depth, inverse = ball_scene()
    free, _ = fused(lat, depth, inverse)
    capped, _ = fused(lat, depth, inverse, max_weight=2.0)
    half, _ = fused(lat, depth, inverse, weight=0.5, max_weight=1.25)
    assert set(np.unique(free[..., 1])) == {0.0, 1.0, 2.0, 3.0}  # of two opposite views at most one sees a voxel
    assert capped[..., 1].max() == 2.0 and np.array_equal(capped[..., 1], np.minimum(free[..., 1], 2.0))
    assert half[..., 1].max() == 1.25 and set(np.unique(half[..., 1])) == {0.0, 0.5, 1.0, 1.25}
    for state in (free, capped, half):
        assert np.abs(state[..., 0]).max() <= 1.0 and state[..., 0].max() == 1.0


def test_an_untouched_voxel_keeps_its_bits():
    lat, depth, inverse = ball_scene()
    rng = np.random.default_rng(2)
    before = rng.uniform(-1, 1, size=lat.dims + (2,)).astype(np.float32)
    before[..., 1] = np.abs(before[..., 1]) * 3
    before[::2] = -0.0
    fresh, _ = fused(lat, depth, inverse)
    after, _ = fused(lat, depth, inverse, state=before)
    untouched = fresh[..., 1] == 0
    assert 1000 < untouched.sum() < untouched.size - 1000  # the ball's inside and the corners no view sees
    assert np.array_equal(after[untouched].view(np.int32), before[untouched].view(np.int32))
    assert np.signbit(after[untouched][:, 0]).any()
    assert (after[~untouched][:, 1] != before[~untouched][:, 1]).all()


def test_the_surface_lies_within_a_fraction_of_a_voxel_of_the_ball():
    """The property this feature exists for.  Zero crossings of val along lattice edges between two known voxels with |t| < 1
    lie, in voxels, less than 0.25 from the sphere on average (the expected quantisation error of the occupancy route) and less
    than 1 at worst; every voxel within half a voxel of the sphere is known.  The restatement gives 0.091 mean, 0.571 worst over
    4230 crossings, and 2622 of 2622 voxels known (profiles/tsdf.md)."""
    lat, depth, inverse = ball_scene()
    state, _ = fused(lat, depth, inverse)
    rec = ref.records(state, BALL_RES, BALL_TRUNC).reshape(lat.dims + (4,))
    c = ref.centres(lat).astype(np.float64)
    t, known = state[..., 0], state[..., 1] > 0
    val = rec[..., 0].astype(np.float64)
    assert np.array_equal(rec[..., 0], np.where(known, np.float32(BALL_TRUNC) * t, np.float32(BALL_TRUNC)))
    usable = known & (np.abs(t) < 1)
    errors = []
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = usable[a] & usable[b] & ((val[a] < 0) != (val[b] < 0))
        s = val[a][cross] / (val[a][cross] - val[b][cross])
        p = c[a][cross] + s[:, None] * (c[b][cross] - c[a][cross])
        errors.append(np.abs(np.linalg.norm(p, axis=1) - BALL_RADIUS) / BALL_RES)
    errors = np.concatenate(errors)
    near = np.abs(np.linalg.norm(c, axis=-1) - BALL_RADIUS) < BALL_RES / 2
    print(f"crossings {errors.size} mean {errors.mean():.4f} max {errors.max():.4f} voxels; near the sphere {near.sum()}, "
          f"known {int((near & known).sum())}")
    assert errors.size > 3000
    assert errors.mean() < 0.25
    assert errors.max() < 1.0
    assert near.sum() > 2000 and (known[near]).all()


def test_records_have_unit_gradients_that_point_out_of_the_ball_and_zeros_where_saturated():
    lat, depth, inverse = ball_scene()
    state, _ = fused(lat, depth, inverse)
    for unknown in (1.0, -1.0):
        rec = ref.records(state, BALL_RES, BALL_TRUNC, unknown_tsdf=unknown).reshape(lat.dims + (4,))
        length = np.linalg.norm(rec[..., 1:].astype(np.float64), axis=-1)
        assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all() and (length == 0).any() and (length > 0).any()
        assert np.abs(rec[..., 0]).max() == np.float32(BALL_TRUNC)
    rec = ref.records(state, BALL_RES, BALL_TRUNC).reshape(lat.dims + (4,))
    assert not rec[0, 0, 0, 1:].any()       # a corner no ray with a return passes: unknown all round
    assert not rec[25, 25, 25, 1:].any()    # the centre: further behind the surface than the band, never updated
    c = ref.centres(lat).astype(np.float64)
    r = np.linalg.norm(c, axis=-1)
    # within a voxel of the sphere, where all six neighbours are known too, the stored normal points out of the ball: every view's
    # distance grows along its ray toward the camera, each camera is on the outer side of the surface it sees, and the average
    # of such fields grows outward.  Nothing sharper follows: a view up to 55 degrees off the normal tilts its share.
    known = np.pad(state[..., 1] > 0, 1)
    around = known[1:-1, 1:-1, 1:-1].copy()
    for axis in range(3):
        around &= np.roll(known, 1, axis)[1:-1, 1:-1, 1:-1] & np.roll(known, -1, axis)[1:-1, 1:-1, 1:-1]
    shell = (np.abs(r - BALL_RADIUS) < BALL_RES) & around
    cosine = (rec[..., 1:][shell] * (c[shell] / r[shell][:, None])).sum(-1)
    assert shell.sum() > 4000 and cosine.min() > 0
    # a weight threshold turns voxels few frames saw into unknown ones
    strict = ref.records(state, BALL_RES, BALL_TRUNC, min_weight=1.0).reshape(lat.dims + (4,))
    once = state[..., 1] == 1.0
    assert once.any() and (strict[..., 0][once] == np.float32(BALL_TRUNC)).all()
