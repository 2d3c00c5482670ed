"""Restatement of the TSDF contract (include/pvamd.h "TSDF integration") for its tests -- TEST INFRASTRUCTURE: tsdf_ref.c compiled
on the fly, and the scenes the CPU and GPU tests share: analytic depth images of a ball and the camera poses that see it."""
import ctypes

import numpy as np

from tests import c_ref

# the branch counters of tsdf_ref.c, in its enum's order
HITS = ("behind", "u_low_edge", "u_high_edge", "u_half", "clamped", "no_return", "too_far", "band_edge", "behind_band",
        "saturated_edge", "updated", "outside")


class Lattice(ctypes.Structure):
    """lattice_t of tsdf_ref.c: the fields of pvamd_grid_t the contract reads."""
    _fields_ = [("fmin", ctypes.c_float * 3), ("fres", ctypes.c_float * 3), ("shape", ctypes.c_int32 * 3)]

    @property
    def dims(self):
        return tuple(self.shape)


def load():
    return c_ref.load("tsdf_ref")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lattice_of(desc):
    """Lattice from anything with pvamd_grid_t's fields (a _lib.GridDesc)."""
    lat = Lattice()
    for k in range(3):
        lat.fmin[k], lat.fres[k], lat.shape[k] = desc.fmin[k], desc.fres[k], desc.shape[k]
    return lat


def make_lattice(shape, lo, res):
    """A lattice whose voxel i of axis k is centred on lo_k + i * res: no library needed."""
    lat = Lattice()
    for k in range(3):
        lat.fmin[k], lat.fres[k], lat.shape[k] = np.float32(lo[k]), np.float32(res), shape[k]
    return lat


def centres(lat):
    """(nx, ny, nz, 3) float32 voxel centres, statement 2."""
    axes = [np.float32(lat.fmin[k]) + np.arange(lat.shape[k], dtype=np.float32) * np.float32(lat.fres[k]) for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)


def integrate(lat, state, depth, inverse, intrinsics, truncation, max_depth=np.inf, weight=1.0, max_weight=np.inf):
    """Statements 1-9 in place on `state` (nx, ny, nz, 2) float32; depth (K, H, W) float32, inverse (K, 3, 4) float32.  Returns
    how often each branch was taken, by name (HITS)."""
    depth = np.ascontiguousarray(depth, np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    inverse = np.ascontiguousarray(inverse, np.float32).reshape(-1, 3, 4)
    K, H, W = depth.shape
    assert inverse.shape[0] == K and state.dtype == np.float32 and state.flags.c_contiguous and state.shape == lat.dims + (2,)
    hits = np.zeros(len(HITS), np.int64)
    fx, fy, cx, cy = intrinsics
    f = ctypes.c_float
    load().tsdf_integrate_ref(ctypes.byref(lat), _p(depth), ctypes.c_int32(K), ctypes.c_int32(H), ctypes.c_int32(W), _p(inverse),
                              f(fx), f(fy), f(cx), f(cy), f(truncation), f(max_depth), f(weight), f(max_weight), _p(state),
                              _p(hits))
    return dict(zip(HITS, hits.tolist()))


def records(state, resolution, truncation, min_weight=0.0, unknown_tsdf=1.0):
    """(n, 4) float32 records of statements 10-12."""
    nx, ny, nz, _ = state.shape
    assert state.dtype == np.float32 and state.flags.c_contiguous
    out = np.empty((nx * ny * nz, 4), np.float32)
    f = ctypes.c_float
    load().tsdf_records_ref(_p(state), ctypes.c_int32(nx), ctypes.c_int32(ny), ctypes.c_int32(nz), f(resolution), f(truncation),
                            f(min_weight), f(unknown_tsdf), _p(out))
    return out


def invert(poses):
    """(K, 3, 4) float32: the rigid inverse of (K, 4, 4) poses in float64, rounded once -- statement by statement what
    pytorch_volumetric_amd.tsdf.camera_from_volume does."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    Rt = poses[:, :3, :3].transpose(0, 2, 1)
    t = poses[:, :3, 3]
    back = -((Rt[:, :, 0] * t[:, None, 0] + Rt[:, :, 1] * t[:, None, 1]) + Rt[:, :, 2] * t[:, None, 2])
    return np.concatenate((Rt, back[:, :, None]), axis=2).astype(np.float32)


# ---------------------------------------------------------------- the scenes the tests share
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """(4, 4) float64 pose of a camera at `eye` looking at `target`: +z forward, x right, y down."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    down = -np.asarray(up, np.float64)
    if abs(np.dot(z, down)) > 0.99:  # looking along the up direction: any other hint will do
        down = np.array([0.0, 1.0, 0.0])
    x = np.cross(down, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose


def wall_frames(ranges, res, K=3, height=48, width=64, axis=None):
    """(depth (K, H, W) float32, poses (K, 4, 4) float64), read-only: the frames of tests/test_tsdf_gpu.py for any lattice, its
    lengths in voxels (at res = 0.25 the same scene): K cameras around and inside the lattice, every one rotated against its
    axes, looking at a rippled wall through its middle; a tenth of the pixels hold what a sensor reports instead of a return
    (0, a negative number, NaN, inf) or a depth past any max_depth below 1000.
    `axis`: the lattice is a line along this axis; the cameras stand beside it, off its middle, and see it obliquely from
    end to end."""
    ranges = np.array(ranges, np.float64)
    centre, reach = ranges.mean(axis=1), np.linalg.norm(ranges[:, 1] - ranges[:, 0]) / 2 + 4.0 * res
    if axis is None:
        eyes = [centre + reach * np.array([0.6, -0.5, 0.62]), centre + 0.2 * reach * np.array([-0.3, 0.4, 0.1]),  # the second: inside
                centre + reach * np.array([-0.45, 0.8, -0.4])]
    else:
        along, beside, third = np.eye(3)[axis], np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]
        eyes = [centre + reach * (0.3 * along + 2.6 * beside + 0.3 * third), centre + reach * (-0.25 * along - 2.5 * beside + 0.4 * third)]
    poses = np.stack([look_at(eyes[k % len(eyes)], centre + 0.4 * res * k) for k in range(K)])
    rows, cols = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    mean = 1.0 if axis is None else 1.03  # beside a line the wall stands a little behind its middle: parts of either end are in front of it
    depth = np.stack([np.linalg.norm(eyes[k % len(eyes)] - centre) * (mean + 0.3 * np.sin(0.3 * cols + k) * np.cos(0.2 * rows)) + 0.2 * res
                      for k in range(K)]).astype(np.float32)
    rng = np.random.default_rng(7)
    kind = rng.integers(0, 50, size=depth.shape)
    for code, value in enumerate((0.0, -1.5, np.nan, np.inf, 1000.0)):
        depth[kind == code] = value
    depth.flags.writeable = poses.flags.writeable = False
    return depth, poses


def axis_views(centre, distance):
    """Six poses looking at `centre` from `distance` along -x, +x, -y, +y, -z, +z."""
    centre = np.asarray(centre, np.float64)
    return np.stack([look_at(centre + sign * distance * np.eye(3)[k], centre) for k in range(3) for sign in (-1.0, 1.0)])


def ball_depth(poses, intrinsics, H, W, centre, radius):
    """(K, H, W) float32 z-depth images of a ball by exact ray-sphere intersection in float64; 0 where the pixel's ray misses."""
    fx, fy, cx, cy = intrinsics
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack(((cols - cx) / fx, (rows - cy) / fy, np.ones_like(cols)), axis=-1)  # z component 1: the parameter is z-depth
    out = np.zeros((len(poses), H, W), np.float32)
    for k, pose in enumerate(np.asarray(poses, np.float64).reshape(-1, 4, 4)):
        d = d_cam @ pose[:3, :3].T
        o = pose[:3, 3] - np.asarray(centre, np.float64)
        a = (d * d).sum(-1)
        b = (d * o).sum(-1)
        disc = b * b - a * (o @ o - radius * radius)
        s = (-b - np.sqrt(np.where(disc >= 0, disc, 0.0))) / a
        out[k] = np.where((disc >= 0) & (s > 0), s, 0.0).astype(np.float32)
    return out
