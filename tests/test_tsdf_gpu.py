"""-m gpu: TSDF fusion on the device, bit for bit against the C restatement of the contract (tests/tsdf_ref.c), through
pv.TSDFVolume and pv.TSDFField, and the leaf it makes in front of ray_cast and refine_poses."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import tsdf as tsdf_module
from tests import helpers as H
from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu

# resolution 0.25 over ranges that start on a multiple of it: voxel centres are exact in float32
RES, TRUNC = 0.25, 0.75
LATTICES = {(2, 2, 2): [(0.0, 0.25), (-1.0, -0.75), (0.5, 0.75)],
            (19, 13, 37): [(0.0, 4.5), (-1.0, 2.0), (0.0, 9.0)],
            (5, 3, 131): [(0.0, 1.0), (0.0, 0.5), (0.0, 32.5)],       # a wave spans several z lines, a z line several waves
            (96, 80, 72): [(-12.0, 11.75), (-10.0, 9.75), (0.0, 17.75)]}  # 552,960 voxels: past the 2048 x 256 streaming cap
HEIGHT, WIDTH = 48, 64
INTRINSICS = (40.0, 36.0, 31.5, 23.5)
assert 96 * 80 * 72 > H.STREAM_GRID_ITEMS


def new_volume(shape, **kwargs):
    kwargs.setdefault("max_weight", math.inf)
    vol = pv.TSDFVolume(RES, LATTICES[shape], truncation=TRUNC, device="cuda", **kwargs)
    assert vol.shape == shape
    return vol


def lattice(vol):
    return ref.lattice_of(vol._grid.voxels._grid_desc())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def state_of(vol):
    return vol._state.cpu().numpy()


@functools.lru_cache(maxsize=None)
def frames(shape, K=3):
    """(depth (K, H, W) float32, poses (K, 4, 4) float64), read-only: K cameras around and inside the lattice, every one rotated
    against its axes, looking at a rippled wall through its middle; a tenth of the pixels hold what a sensor reports instead of
    a return (0, a negative number, NaN, inf) or a depth past the max_depth the tests use."""
    ranges = np.array(LATTICES[shape])
    centre, reach = ranges.mean(axis=1), np.linalg.norm(ranges[:, 1] - ranges[:, 0]) / 2 + 1.0
    eyes = [centre + reach * np.array([0.6, -0.5, 0.62]), centre + 0.2 * reach * np.array([-0.3, 0.4, 0.1]),  # the second: inside
            centre + reach * np.array([-0.45, 0.8, -0.4])]
    poses = np.stack([ref.look_at(eyes[k % 3], centre + 0.1 * k) for k in range(K)])
    rows, cols = np.meshgrid(np.arange(HEIGHT), np.arange(WIDTH), indexing="ij")
    depth = np.stack([np.linalg.norm(eyes[k % 3] - centre) * (1.0 + 0.3 * np.sin(0.3 * cols + k) * np.cos(0.2 * rows)) + 0.05
                      for k in range(K)]).astype(np.float32)
    rng = np.random.default_rng(7)
    kind = rng.integers(0, 50, size=depth.shape)
    for code, value in enumerate((0.0, -1.5, np.nan, np.inf, 1000.0)):
        depth[kind == code] = value
    depth.flags.writeable = poses.flags.writeable = False
    return depth, poses


MAX_DEPTH = 500.0


def integrate_both(vol, want, depth, poses, **kwargs):
    """One integrate() on the device and the same call on the restatement's state `want`; returns the restatement's branch counts."""
    vol.integrate(torch.from_numpy(np.array(depth)), INTRINSICS, torch.from_numpy(np.array(poses)).cuda(), **kwargs)
    return ref.integrate(lattice(vol), want, depth, ref.invert(poses), INTRINSICS, TRUNC, max_weight=vol.max_weight, **kwargs)


def assert_same_state(vol, want):
    got = state_of(vol)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


# ---------------------------------------------------------------- integration
def test_the_pose_inverse_on_the_device_is_the_restatement():
    _, poses = frames((19, 13, 37))
    got = tsdf_module.camera_from_volume(torch.from_numpy(np.array(poses)).cuda())
    assert got.is_cuda and np.array_equal(bits(got.cpu().numpy()), bits(ref.invert(poses)))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("shape", list(LATTICES))
def test_state_bit_for_bit_and_frames_in_one_call_equal_sequential_calls(shape, K):
    depth, poses = frames(shape)
    depth, poses = depth[:K], poses[:K]
    vol, want = new_volume(shape), np.zeros(shape + (2,), np.float32)
    hits = integrate_both(vol, want, depth, poses, max_depth=MAX_DEPTH)
    assert_same_state(vol, want)
    assert hits["updated"] > 0
    if shape != (2, 2, 2):
        assert hits["outside"] > 0 and hits["no_return"] > 0 and hits["too_far"] > 0 and hits["behind_band"] > 0
        assert 0 < (want[..., 1] == 0).sum() < want[..., 1].size
        assert (want[..., 0] == 1.0).any() and (np.abs(want[..., 0]) < 1.0).any() and (want[..., 0] < 0).any()
    if K == 3:
        assert shape == (2, 2, 2) or hits["behind"] > 0  # the second camera is inside the volume
        step = new_volume(shape)
        for k in range(K):  # (H, W) with (4, 4), and (1, H, W) with (1, 4, 4)
            d, p = (depth[k], poses[k]) if k % 2 else (depth[k:k + 1], poses[k:k + 1])
            step.integrate(torch.from_numpy(np.array(d)).cuda(), INTRINSICS, torch.from_numpy(np.array(p)), max_depth=MAX_DEPTH)
        assert_same_state(step, want)
    assert torch.equal(vol.tsdf, vol._state[..., 0]) and torch.equal(vol.weight, vol._state[..., 1])
    vol.reset()
    assert not vol._state.view(torch.int32).any()


def test_depth_of_any_real_dtype_is_scaled_on_the_device():
    shape = (19, 13, 37)
    _, poses = frames(shape)
    counts = np.random.default_rng(3).integers(-2, 60, size=(3, HEIGHT, WIDTH)).astype(np.int16)  # in units of a voxel
    vol, want = new_volume(shape), np.zeros(shape + (2,), np.float32)
    vol.integrate(torch.from_numpy(counts), torch.tensor([[40.0, 0.0, 31.5], [0.0, 36.0, 23.5], [0.0, 0.0, 1.0]]),
                  torch.from_numpy(np.array(poses)).float(), depth_scale=0.25)
    hits = ref.integrate(lattice(vol), want, counts.astype(np.float32) * np.float32(0.25), ref.invert(poses.astype(np.float32)),
                         INTRINSICS, TRUNC)
    assert_same_state(vol, want)
    assert hits["updated"] > 0 and hits["no_return"] > 0
    same = new_volume(shape)
    same.integrate(torch.from_numpy(counts).double().cuda() * 0.25, INTRINSICS, torch.from_numpy(np.array(poses)).float().cuda())
    assert_same_state(same, want)


def edge_frames():
    """A camera on a lattice point of the (19, 13, 37) lattice, its axes along the lattice's, fx and fy four pixels per voxel at
    depth 1: voxel centres project exactly onto pixel boundaries, u = j + 0.5, and onto both ends of the image, -0.5 and W - 0.5.
    The wall is at depth 2, so the centres at depth 2.75 and 1.25 lie exactly on the two ends of the band; five columns report
    no return or one past max_depth below the third row."""
    pose = np.eye(4)
    pose[:3, 3] = (1.0, 0.0, 1.0)
    depth = np.full((1, 6, 8), 2.0, np.float32)
    for col, value in enumerate((0.0, -1.0, np.nan, np.inf, 100.0), start=1):
        depth[0, 3:, col] = value
    return depth, pose[None], (4.0, 4.0, 0.5, 0.5)


def test_projection_and_depth_edge_cases():
    shape = (19, 13, 37)
    depth, poses, intrinsics = edge_frames()
    vol, want = new_volume(shape), np.zeros(shape + (2,), np.float32)
    vol.integrate(torch.from_numpy(depth), intrinsics, torch.from_numpy(poses), max_depth=50.0)
    hits = ref.integrate(lattice(vol), want, depth, ref.invert(poses), intrinsics, TRUNC, max_depth=50.0)
    for branch in ("u_half", "u_low_edge", "u_high_edge", "behind", "outside", "no_return", "too_far", "band_edge", "saturated_edge",
                   "behind_band", "updated"):
        assert hits[branch] > 0, branch  # the restatement really takes the branch
    assert_same_state(vol, want)
    # the camera's own lattice point (4, 4, 4): depth 1.0 is z index 8, the wall z index 12, the band's ends 9 and 15
    assert want[4, 4, 12, 0] == 0.0 and want[4, 4, 12, 1] == 1.0
    assert want[4, 4, 15, 0] == -1.0 and want[4, 4, 15, 1] == 1.0 and want[4, 4, 16, 1] == 0.0  # sdf == -truncation is inside
    assert want[4, 4, 9, 0] == 1.0 and want[4, 4, 10, 0] < 1.0
    assert want[3, 4, 8, 1] == 1.0 and want[11, 4, 8, 1] == 0.0  # u == -0.5 is inside the image, u == W - 0.5 is not
    assert want[4, 4, 4, 1] == 0.0 and want[4, 4, 3, 1] == 0.0   # p_z == 0 and p_z < 0


def test_the_weight_cap_and_a_prefilled_state():
    shape = (19, 13, 37)
    depth, poses = frames(shape)
    vol, want = new_volume(shape, max_weight=2.0), np.zeros(shape + (2,), np.float32)
    integrate_both(vol, want, depth, poses)
    integrate_both(vol, want, depth[::-1], poses[::-1], weight=0.75)
    assert_same_state(vol, want)
    assert want[..., 1].max() == 2.0 and (want[..., 1] == 2.0).sum() > 100
    # a state someone else wrote: a pattern, -0.0 in every other x slab; what no frame reaches keeps its bits
    rng = np.random.default_rng(11)
    before = rng.uniform(-1, 1, size=shape + (2,)).astype(np.float32)
    before[..., 1] = np.abs(before[..., 1]) * 1.5
    before[::2] = -0.0
    vol._state.copy_(torch.from_numpy(before))
    want = before.copy()
    hits = integrate_both(vol, want, depth[:1], poses[:1])
    assert_same_state(vol, want)
    untouched = bits(want) == bits(before)
    assert hits["updated"] > 0 and untouched.all(axis=-1).sum() > 100 and np.signbit(state_of(vol)[..., 0]).any()


def test_two_replays_of_a_captured_integrate_equal_two_eager_calls():
    shape = (19, 13, 37)
    depth, poses = frames(shape)
    depth_dev, poses_dev = torch.from_numpy(np.array(depth)).cuda(), torch.from_numpy(np.array(poses)).cuda()
    eager, captured = new_volume(shape, max_weight=5.0), new_volume(shape, max_weight=5.0)
    for _ in range(2):
        eager.integrate(depth_dev, INTRINSICS, poses_dev, max_depth=MAX_DEPTH)
    captured.integrate(depth_dev, INTRINSICS, poses_dev, max_depth=MAX_DEPTH)  # warm: the library is loaded before the capture
    captured.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.integrate(depth_dev, INTRINSICS, poses_dev, max_depth=MAX_DEPTH)
    captured.reset()  # what the capture itself ran, if anything, is forgotten
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert eager.weight.max() == 5.0
    assert torch.equal(eager._state.view(torch.int32), captured._state.view(torch.int32))


# ---------------------------------------------------------------- records
@pytest.mark.parametrize("unknown, min_weight", [("free", 0.0), ("occupied", 0.0), ("free", 1.0), ("occupied", 2.5)])
@pytest.mark.parametrize("shape", list(LATTICES))
def test_records_bit_for_bit(shape, unknown, min_weight):
    depth, poses = frames(shape)
    vol, state = new_volume(shape), np.zeros(shape + (2,), np.float32)
    integrate_both(vol, state, depth, poses, max_depth=MAX_DEPTH)
    want = ref.records(state, RES, TRUNC, min_weight=min_weight, unknown_tsdf=1.0 if unknown == "free" else -1.0)
    if not (want[:, 0] <= 0).any():
        with pytest.raises(ValueError):
            pv.TSDFField(vol, unknown=unknown, min_weight=min_weight)
        assert shape == (2, 2, 2)
        return
    field = pv.TSDFField(vol, unknown=unknown, min_weight=min_weight)
    got = field._records.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    if shape == (2, 2, 2):
        return
    rec, known = want.reshape(shape + (4,)), state[..., 1] > min_weight
    length = np.linalg.norm(rec[..., 1:].astype(np.float64), axis=-1)
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all()
    assert (length == 0).any()                                           # flat neighbourhoods: zeros
    border = np.ones(shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert min_weight > 0 or (length[border] > 0).any()                  # one-sided differences at the border
    beside_unknown = known[:, :, 1:] & ~known[:, :, :-1]
    assert beside_unknown.any() and (length[:, :, 1:][beside_unknown] > 0).any()  # known voxels next to unknown ones
    assert (rec[..., 0][~known] == np.float32(TRUNC if unknown == "free" else -TRUNC)).all()
    # the field answers with its records: the nearest voxel's inside the lattice
    idx = np.array([[1, 1, 3], [shape[0] - 2, 1, shape[2] - 2], [shape[0] // 2, 1, shape[2] // 2]])
    pts = torch.from_numpy(ref.centres(lattice(vol))[tuple(idx.T)]).cuda()
    val, grad = field(pts)
    flat = np.ravel_multi_index(tuple(idx.T), shape)
    assert np.array_equal(bits(val.cpu().numpy()), bits(want[flat, 0]))
    assert np.array_equal(bits(grad.cpu().numpy()), bits(want[flat, 1:]))


def test_the_bounding_box_is_that_of_the_voxels_at_or_inside_the_surface_and_a_field_is_a_snapshot():
    shape = (19, 13, 37)
    depth, poses = frames(shape)
    vol = new_volume(shape)
    vol.integrate(torch.from_numpy(np.array(depth)), INTRINSICS, torch.from_numpy(np.array(poses)), max_depth=MAX_DEPTH)
    field = pv.TSDFField(vol)
    rec = field._records.cpu().numpy().reshape(shape + (4,))
    index = np.argwhere(rec[..., 0] <= 0)
    lo = np.array(LATTICES[shape])[:, 0] + index.min(axis=0) * RES - RES / 2
    hi = np.array(LATTICES[shape])[:, 0] + index.max(axis=0) * RES + RES / 2
    assert np.array_equal(field.surface_bounding_box().numpy(), np.stack((lo, hi), axis=1))
    assert np.array_equal(field.surface_bounding_box(padding=0.5).numpy(), np.stack((lo - 0.5, hi + 0.5), axis=1))
    kept = field._records.clone()
    vol.integrate(torch.from_numpy(np.array(depth)), INTRINSICS, torch.from_numpy(np.array(poses)), weight=3.0)
    vol.reset()
    assert torch.equal(field._records.view(torch.int32), kept.view(torch.int32))
    with pytest.raises(ValueError):
        pv.TSDFField(vol)  # a fresh volume: nothing at or inside a surface


# ---------------------------------------------------------------- the C ABI
def test_argument_errors_of_the_entry_points():
    lib = _lib.load()
    E_NULL, E_SHAPE, E_ALIGN, E_MODE = (_lib.H[f"PVAMD_E_{name}"] for name in ("NULL", "SHAPE", "ALIGN", "MODE"))
    vol = new_volume((5, 3, 131))
    desc = ctypes.byref(vol._grid.voxels._grid_desc())
    depth = torch.ones((2, 4, 6), dtype=torch.float32, device="cuda")
    poses = tsdf_module.camera_from_volume(torch.eye(4).expand(2, 4, 4)).cuda()
    state = torch.zeros((5 * 3 * 131 * 2 + 2,), dtype=torch.float32, device="cuda")
    good = dict(grid=desc, depth=_lib.ptr(depth), K=2, H=4, W=6, poses=_lib.ptr(poses), fx=4.0, fy=4.0, cx=2.5, cy=1.5,
                truncation=0.75, max_depth=math.inf, weight=1.0, max_weight=math.inf, state=_lib.ptr(state))

    def integrate(**changes):
        return lib.pvamd_tsdf_integrate(*{**good, **changes}.values(), _lib.stream_ptr())

    for changes in (dict(K=-1), dict(H=0), dict(W=0), dict(K=2, H=2 ** 15, W=2 ** 15)):
        assert integrate(**changes) == E_SHAPE, changes
    for axis, count in ((2, 2049), (0, 1)):
        wide = _lib.GridDesc.from_buffer_copy(vol._grid.voxels._grid_desc())
        wide.shape[axis] = count
        assert integrate(grid=ctypes.byref(wide)) == E_SHAPE
    for name in ("grid", "depth", "poses", "state"):
        assert integrate(**{name: None}) == E_NULL, name
    for name, bad in (("fx", (0.0, -1.0, math.nan, math.inf)), ("fy", (0.0, math.nan)), ("cx", (math.nan, math.inf)),
                      ("cy", (-math.inf,)), ("truncation", (0.0, -1.0, math.nan, math.inf)), ("weight", (0.0, math.nan, math.inf)),
                      ("max_depth", (0.0, -1.0, math.nan)), ("max_weight", (0.0, -2.0, math.nan))):
        for value in bad:
            assert integrate(**{name: value}) == E_MODE, (name, value)
    assert integrate(state=_lib.ptr(state[1:])) == E_ALIGN
    assert integrate(K=0, depth=None, poses=None, state=None) == 0  # no frames: nothing is launched, nothing is needed
    assert integrate(max_depth=math.inf, max_weight=math.inf) == 0
    records = torch.zeros((5 * 3 * 131 * 4 + 4,), dtype=torch.float32, device="cuda")
    fine = dict(state=_lib.ptr(state), nx=5, ny=3, nz=131, resolution=0.25, truncation=0.75, min_weight=0.0, unknown=1.0,
                records=_lib.ptr(records))

    def make_records(**changes):
        return lib.pvamd_tsdf_records(*{**fine, **changes}.values(), _lib.stream_ptr())

    for changes in (dict(nx=1), dict(ny=0), dict(nz=2049), dict(nx=2048, ny=2048, nz=2048)):
        assert make_records(**changes) == E_SHAPE, changes
    for changes in (dict(resolution=0.0), dict(resolution=math.inf), dict(truncation=-1.0), dict(truncation=math.nan),
                    dict(min_weight=math.nan), dict(unknown=0.0), dict(unknown=0.5), dict(unknown=math.nan)):
        assert make_records(**changes) == E_MODE, changes
    assert make_records(state=None) == E_NULL and make_records(records=None) == E_NULL
    assert make_records(state=_lib.ptr(state[1:])) == E_ALIGN and make_records(records=_lib.ptr(records[2:])) == E_ALIGN
    assert make_records(unknown=-1.0, min_weight=math.inf) == 0
    torch.cuda.synchronize()
    assert (records[:5 * 3 * 131 * 4].reshape(-1, 4)[:, 0] == -0.75).all() and not records[-4:].any()


# ---------------------------------------------------------------- the leaf in front of its consumers
def camera_rays(pose, intrinsics, height, width):
    """(origins, unit directions, z component of each direction in the camera) of the pixels' rays, float32 on the GPU."""
    fx, fy, cx, cy = intrinsics
    rows, cols = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    d = np.stack(((cols - cx) / fx, (rows - cy) / fy, np.ones_like(cols)), axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    world = d @ pose[:3, :3].T
    origins = np.broadcast_to(pose[:3, 3], world.shape)
    return (torch.from_numpy(np.ascontiguousarray(origins)).float().cuda(), torch.from_numpy(world).float().cuda(),
            torch.from_numpy(d[..., 2]).float().cuda())


def test_depth_rendered_from_a_cache_fuses_into_a_leaf_that_ray_cast_and_refine_poses_take():
    radius, res, ranges, intrinsics = 0.3, 0.02, [(-0.5, 0.5)] * 3, (60.0, 60.0, 31.5, 23.5)
    ball = pv.CachedSDF("ball", res, ranges, pv.SphereSDF(radius), device="cuda", cache_path=None)
    poses = ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = []
    for pose in poses:  # 64 x 48 rays per pose: the model depth ray_cast renders
        o, d, dz = camera_rays(pose, intrinsics, 48, 64)
        cast = ball.ray_cast(o, d)
        depth.append(torch.where(cast.status == pv.RAY_HIT, cast.t * dz, torch.zeros_like(cast.t)))
    depth = torch.stack(depth)
    assert depth.shape == (6, 48, 64) and (depth > 0).sum() > 6 * 500
    vol = pv.TSDFVolume(res, ranges, truncation=0.06, device="cuda")
    vol.integrate(depth, intrinsics, torch.from_numpy(poses).cuda())
    assert vol.shape == (51, 51, 51) and (vol.weight > 0).any() and (vol.tsdf < 0).any()
    field = pv.TSDFField(vol)
    scene = vol.to_sdf("scene")
    assert torch.equal(scene._packed.view(torch.int32), field._records.view(torch.int32))  # the records, taken as they are
    smooth = vol.to_sdf("scene", interpolation="trilinear")
    assert smooth.interpolation == "trilinear" and torch.equal(smooth._packed.view(torch.int32), field._records.view(torch.int32))
    # a seventh pose: its central rays hit, inside the band round the ball (the field says nothing sharper: it is truncated)
    eye = np.array([0.8, 0.5, 0.4])
    o, d, _ = camera_rays(ref.look_at(eye, (0.0, 0.0, 0.0)), intrinsics, 48, 64)
    for sdf in (scene, smooth):
        cast = sdf.ray_cast(o, d, max_steps=256)
        centre = cast.status[22:26, 30:34]
        assert (centre == pv.RAY_HIT).all() and (cast.status == pv.RAY_HIT).sum() > 300
        assert (cast.t[22:26, 30:34] - (np.linalg.norm(eye) - radius)).abs().max() < 0.06
    # tracking: points on the ball, seen from a pose that is a little off
    g = torch.Generator().manual_seed(4)
    pts = torch.nn.functional.normalize(torch.randn(600, 3, generator=g), dim=-1).cuda() * radius
    off = torch.eye(4, device="cuda").repeat(2, 1, 1)
    off[0, :3, 3] = torch.tensor([0.012, -0.008, 0.01])
    off[1, :3, 3] = torch.tensor([-0.02, 0.0, 0.015])
    for sdf in (scene, smooth):
        fit = pv.refine_poses(off, pts, sdf, iterations=5)
        assert torch.isfinite(fit.cost).all() and (fit.cost <= fit.initial_cost).all() and (fit.initial_cost > 0).all()
