"""TSDF fusion of depth images: a truncated signed distance volume over a VoxelGrid's lattice that every depth frame is averaged
into, in the manner of Curless & Levoy and KinectFusion (include/pvamd.h "TSDF integration", csrc/tsdf.hip).

The reference has no counterpart: its voxel.py stops at the containers.  OccupancyMap -> distance_transform puts the surface on
voxel faces; a TSDFVolume keeps it between the voxels, where the depth images saw it, and hands it to the same consumers:
ray_cast renders the model depth, refine_poses tracks against it, and integrate() is the step between them.
"""
import math
import numbers

import torch

from pytorch_volumetric_amd import _lib, surface
from pytorch_volumetric_amd._lattice import lattice_grid, positive, positive_finite, real
from pytorch_volumetric_amd.occupancy import OccupancySDF
from pytorch_volumetric_amd.occupancy_map import _check_unknown
from pytorch_volumetric_amd.redistance import _check_range, _redistance_records
from pytorch_volumetric_amd.sdf import CachedSDF

MIN_AXIS, MAX_AXIS = _lib.TSDF_MIN_AXIS, _lib.LATTICE_MAX_AXIS  # include/pvamd.h "TSDF integration"
MAX_PIXELS = _lib.TSDF_MAX_PIXELS  # K * H * W of one call


def _check_min_weight(min_weight):
    min_weight = real("min_weight", min_weight)
    if math.isnan(min_weight):
        raise ValueError("min_weight must not be NaN")
    return min_weight


def _check_far_field(far_field, max_distance):
    """max_distance as a float; it means something only with far_field=True."""
    if type(far_field) is not bool:
        raise TypeError(f"far_field must be a bool, got {type(far_field).__name__}")
    _, max_distance = _check_range(0.0, max_distance)
    if not far_field and max_distance != math.inf:
        raise ValueError("max_distance limits the far field: it needs far_field=True")
    return max_distance


def _check_intrinsics(intrinsics):
    """(fx, fy, cx, cy) as Python floats from four reals or a 3 x 3 matrix (read on the host)."""
    if torch.is_tensor(intrinsics):
        intrinsics = intrinsics.detach().cpu().tolist()
    elif hasattr(intrinsics, "tolist"):
        intrinsics = intrinsics.tolist()
    intrinsics = list(intrinsics)
    if len(intrinsics) == 4 and all(isinstance(v, numbers.Real) for v in intrinsics):
        fx, fy, cx, cy = (float(v) for v in intrinsics)
    elif len(intrinsics) == 3 and all(hasattr(row, "__len__") and len(row) == 3 for row in intrinsics):
        fx, fy, cx, cy = float(intrinsics[0][0]), float(intrinsics[1][1]), float(intrinsics[0][2]), float(intrinsics[1][2])
    else:
        raise ValueError("intrinsics must be (fx, fy, cx, cy) or a 3 x 3 matrix")
    if not all(math.isfinite(v) for v in (fx, fy, cx, cy)) or fx <= 0 or fy <= 0:
        raise ValueError(f"intrinsics must be finite with fx, fy > 0, got fx={fx} fy={fy} cx={cx} cy={cy}")
    return fx, fy, cx, cy


def camera_from_volume(camera_pose):
    """(K, 3, 4) float32 on the pose's own device: the rigid inverse (R^T, -R^T t) of (K, 4, 4) or (4, 4) camera poses, worked out
    in float64 and rounded once.  Elementwise products and sums in a fixed order, so every device gives the same bits.  A pose
    that is not rigid is the caller's problem: nothing here looks at the values."""
    pose = camera_pose if torch.is_tensor(camera_pose) else torch.as_tensor(camera_pose)
    pose = pose.detach().to(torch.float64).reshape(-1, 4, 4)
    Rt = pose[:, :3, :3].transpose(1, 2)
    t = pose[:, :3, 3]
    back = -((Rt[:, :, 0] * t[:, None, 0] + Rt[:, :, 1] * t[:, None, 1]) + Rt[:, :, 2] * t[:, None, 2])
    return torch.cat((Rt, back[:, :, None]), dim=2).to(torch.float32).contiguous()


def camera_rays(intrinsics, height, width, camera_pose=None):
    """(origins, directions) of a pinhole camera's pixel rays in the convention integrate() fixes: pixel (row, col) is centred on
    (u, v) = (col, row) and the camera looks along +z with x right and y down, so the ray of a pixel points along
    ((u - cx) / fx, (v - cy) / fy, 1), normalised.

    :param intrinsics: (fx, fy, cx, cy) or a 3 x 3 matrix
    :param camera_pose: None (the rays stay in the camera frame), (4, 4) or (K, 4, 4): the camera's pose in the target frame
    :return: directions (K,) H x W x 3 of unit length and origins (K,) 1 x 1 x 3 that broadcast against them (zeros without a
        pose), in the pose's floating dtype on the pose's device (float32 on the CPU without one).  Plain torch: elementwise
        products and sums in a fixed order, so every device gives the same bits."""
    origins, directions, _ = _pinhole(intrinsics, height, width, camera_pose)
    return origins, directions


def _pinhole(intrinsics, height, width, camera_pose):
    """camera_rays' (origins, directions) and the unit directions in the camera frame, (H, W, 3), that they were turned from."""
    fx, fy, cx, cy = _check_intrinsics(intrinsics)
    for name, n in (("height", height), ("width", width)):
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
            raise ValueError(f"{name} must be a positive integer, got {n!r}")
    pose = None
    if camera_pose is not None:
        pose = camera_pose if torch.is_tensor(camera_pose) else torch.as_tensor(camera_pose)
        if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) != (4, 4):
            raise ValueError(f"camera_pose must be (4, 4) or (K, 4, 4), got {tuple(pose.shape)}")
        pose = pose.detach()
        if not pose.dtype.is_floating_point:
            pose = pose.to(torch.float32)
    dtype, device = (torch.float32, torch.device("cpu")) if pose is None else (pose.dtype, pose.device)
    x = ((torch.arange(width, dtype=dtype, device=device) - cx) / fx)[None, :].expand(height, width)
    y = ((torch.arange(height, dtype=dtype, device=device) - cy) / fy)[:, None].expand(height, width)
    length = torch.sqrt((x * x + y * y) + 1.0)
    local = torch.stack((x / length, y / length, 1.0 / length), dim=-1)
    if pose is None:
        return torch.zeros((1, 1, 3), dtype=dtype, device=device), local, local
    lx, ly, lz = local[..., 0], local[..., 1], local[..., 2]
    rot = pose[..., :3, :3, None, None]  # (K,) 3 x 3 x 1 x 1
    directions = torch.stack([(rot[..., i, 0, :, :] * lx + rot[..., i, 1, :, :] * ly) + rot[..., i, 2, :, :] * lz for i in range(3)],
                             dim=-1)
    return pose[..., None, None, :3, 3], directions, local


def _check_frames(depth, intrinsics, camera_pose, max_depth, weight, depth_scale):
    """The argument errors of integrate, raised before a GPU is asked for."""
    depth = depth if torch.is_tensor(depth) else torch.as_tensor(depth)
    pose = camera_pose if torch.is_tensor(camera_pose) else torch.as_tensor(camera_pose)
    if depth.is_complex():
        raise TypeError(f"depth must have a real dtype, got {depth.dtype}")
    if depth.dim() not in (2, 3):
        raise ValueError(f"depth must be (H, W) or (K, H, W), got {tuple(depth.shape)}")
    if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) != (4, 4):
        raise ValueError(f"camera_pose must be (4, 4) or (K, 4, 4), got {tuple(pose.shape)}")
    K = 1 if depth.dim() == 2 else depth.shape[0]
    if (1 if pose.dim() == 2 else pose.shape[0]) != K:
        raise ValueError(f"depth holds {K} frame(s) and camera_pose {1 if pose.dim() == 2 else pose.shape[0]}: one pose per frame")
    H, W = depth.shape[-2:]
    if K and (H < 1 or W < 1):
        raise ValueError(f"depth images need at least one pixel, got {tuple(depth.shape)}")
    if K * H * W > MAX_PIXELS:
        raise ValueError(f"one call takes fewer than 2^31 pixels, got {tuple(depth.shape)}")
    fx, fy, cx, cy = _check_intrinsics(intrinsics)
    return (depth, pose, K, H, W, (fx, fy, cx, cy), positive("max_depth", max_depth), positive_finite("weight", weight),
            float(depth_scale))


class TSDFVolume:
    """A truncated signed distance volume over the lattice of a float32 VoxelGrid(resolution, range_per_dim).

    integrate() averages depth frames into it: per voxel the running mean of min(1, (depth - z) / truncation) over the frames that
    saw the voxel in front of, or less than the truncation behind, a surface.  The state is one (nx, ny, nz, 2) tensor of
    (tsdf, weight) pairs; everything stays on the GPU and nothing carries an autograd graph.
    """

    def __init__(self, resolution, range_per_dim, truncation, device="cuda", max_weight=64.):
        """
        :param resolution: side length of a voxel
        :param range_per_dim: three (low, high) pairs, snapped to whole voxels like a VoxelGrid's
        :param truncation: the width of the band either side of a surface in which distances are kept, in world units; a few
            voxels.  Voxels further behind a surface than this are not updated by that frame.
        :param max_weight: where a voxel's weight stops growing: what bounds how long the volume takes to follow a scene that
            changed.  inf: a plain mean over every frame.
        """
        # the lattice: a VoxelGrid's descriptor.  On the meta device the grid has a shape and no storage; the state below is the volume
        self._grid = lattice_grid(resolution, range_per_dim, "a TSDFVolume", MIN_AXIS, "meta")
        self.truncation = positive_finite("truncation", truncation)
        self.max_weight = positive("max_weight", max_weight)
        self.resolution, self.range_per_dim = self._grid.resolution, range_per_dim
        self.device = torch.device(device)
        if self.device.type == "cuda":
            _lib.require_gpu()
        self._state = torch.zeros(tuple(self._grid.get_voxel_values().shape) + (2,), dtype=torch.float32, device=self.device)

    @property
    def tsdf(self):
        """(nx, ny, nz) float32 view of the state: the averaged distance in units of the truncation, in [-1, 1]."""
        return self._state[..., 0]

    @property
    def weight(self):
        """(nx, ny, nz) float32 view of the state: the accumulated weight, 0 where no frame reached."""
        return self._state[..., 1]

    @property
    def shape(self):
        return tuple(self._state.shape[:3])

    def reset(self):
        """Forget every frame."""
        self._state.zero_()

    def integrate(self, depth, intrinsics, camera_pose, max_depth=math.inf, weight=1.0, depth_scale=1.0):
        """Average K depth frames into the volume, in order, in one pass over it: bit for bit what K calls of one frame give.

        :param depth: (H, W) or (K, H, W), any real dtype: z-depth along the optical axis (not range), times `depth_scale` in
            world units.  Zero, negative, NaN and infinite depths mean "no return".
        :param intrinsics: (fx, fy, cx, cy) or a 3 x 3 matrix, for every frame of the call; pixel (row, col) is centred on
            (u, v) = (col, row)
        :param camera_pose: (4, 4) or (K, 4, 4): the camera's pose in the volume's frame (volume_from_camera); the camera looks
            along +z, x right, y down.  Inverted rigidly on its own device: poses on the GPU never visit the host.
        :param max_depth: returns further than this are ignored
        :param weight: what one frame adds to a voxel's weight
        No frames: a no-op.  One launch; nothing comes back to the host."""
        depth, pose, K, H, W, (fx, fy, cx, cy), max_depth, weight, depth_scale = _check_frames(
            depth, intrinsics, camera_pose, max_depth, weight, depth_scale)
        if K == 0:
            return
        if self.device.type != "cuda":
            raise _lib.PvamdError(f"TSDF integration runs on the GPU and this volume lives on {self.device}; there is no CPU fallback")
        depth = depth.detach().to(device=self.device).to(torch.float32)
        if depth_scale != 1.0:
            depth = depth * depth_scale
        depth = depth.contiguous()
        inverse = camera_from_volume(pose).to(device=self.device)
        with _lib.on_device(self.device):
            _lib.call("pvamd_tsdf_integrate", self._grid.voxels._grid_desc(), depth, K, H, W, inverse, fx, fy, cx, cy,
                      self.truncation, max_depth, weight, self.max_weight, self._state)

    def to_sdf(self, name, unknown="free", min_weight=0.0, interpolation="nearest", far_field=False, max_distance=math.inf):
        """A CachedSDF over the volume's lattice whose records are TSDFField(self, unknown, min_weight, far_field, max_distance)'s,
        taken as they are and not written to a cache file: a snapshot that can be ray-cast, composed with a robot or used for pose
        refinement like any mesh cache.  Without far_field=True its values are truncated: never further from zero than the
        truncation, with a zero gradient beyond it."""
        field = TSDFField(self, unknown=unknown, min_weight=min_weight, far_field=far_field, max_distance=max_distance)
        return CachedSDF(name, field.resolution, field.ranges, field, device=self.device, cache_path=None, interpolation=interpolation)

    def extract_mesh(self, min_weight=0.0, level=0.0, normals=True):
        """The surface the volume has seen as a Surface (vertices, faces, normals on the GPU): naive surface nets
        (surface.extract_surface) over the truncated records (include/pvamd.h "TSDF integration" 10-12, unknown space as free)
        with only the voxels whose weight exceeds `min_weight` usable, so that nothing is meshed between seen and unseen space.
        normals=True interpolates unit normals from the records' gradients.  One synchronisation, to size the result."""
        min_weight = _check_min_weight(min_weight)
        level, normals = surface.check_level(level), surface.check_normals(normals)
        surface.check_shape(self.shape, "the volume")
        if self.device.type != "cuda":
            raise _lib.PvamdError(f"a mesh is extracted on the GPU and this volume lives on {self.device}; there is no CPU fallback")
        nx, ny, nz = self.shape
        records = torch.empty((nx * ny * nz, 4), dtype=torch.float32, device=self.device)
        with _lib.on_device(self.device):
            _lib.call("pvamd_tsdf_records", self._state, nx, ny, nz, self.resolution, self.truncation, min_weight, 1.0, records)
            valid = (self.weight > min_weight).to(torch.uint8).contiguous().reshape(-1)
            return surface.surface_of_records(self._grid.voxels._grid_desc(), records, valid, level, normals)


class TSDFField(OccupancySDF):
    """The truncated signed distance field of a TSDFVolume as an ObjectFrameSDF: value truncation * tsdf and a unit gradient by
    central differences per voxel (include/pvamd.h "TSDF integration" 10-12), worked out once at construction, then answered like a
    nearest-mode BOUNDING_BOX CachedSDF over the volume's lattice (OccupancySDF's descriptor and kernels).  A snapshot: later
    frames do not reach it.  A CachedSDF over the same lattice takes its records as they are.

    far_field=True redistances those records (include/pvamd.h "Redistancing", band = truncation): a voxel whose |value| is below
    the truncation keeps its record bit for bit, every other voxel -- unknown space under either rule included -- gets the
    Euclidean distance to the nearest zero crossing of the values along a lattice edge, with the sign it had and a unit gradient.
    The two meet at |value| = truncation with a step, up to about a voxel where the surface was seen obliquely: projective
    distances inside, Euclidean outside (profiles/redistance.md)."""

    def __init__(self, volume, unknown="free", min_weight=0.0, far_field=False, max_distance=math.inf):
        """
        :param volume: a TSDFVolume
        :param unknown: what a voxel whose weight is not above `min_weight` counts as: "free" (value +truncation) or "occupied"
            (-truncation, what a planner that must not enter unseen space wants)
        :param min_weight: a voxel is known when its weight exceeds this
        :param far_field: False: the truncated field.  True: Euclidean distances beyond the truncation
        :param max_distance: with far_field=True: voxels further than this from the surface read +/-max_distance with a zero
            gradient, which also bounds the work in empty space (inf: no limit)
        """
        _check_unknown(unknown)
        min_weight = _check_min_weight(min_weight)
        max_distance = _check_far_field(far_field, max_distance)
        if volume.device.type != "cuda":
            raise _lib.PvamdError(f"a TSDFField is worked out on the GPU and this volume lives on {volume.device}; there is no CPU fallback")
        self.signed = True
        self.unknown, self.min_weight, self.truncation = unknown, min_weight, volume.truncation
        self.far_field, self.max_distance = far_field, max_distance
        nx, ny, nz = volume.shape
        records = torch.empty((nx * ny * nz, 4), dtype=torch.float32, device=volume.device)
        self._sites = self._squared = None
        with _lib.on_device(volume.device):
            _lib.call("pvamd_tsdf_records", volume._state, nx, ny, nz, volume.resolution, volume.truncation, min_weight,
                      1.0 if unknown == "free" else -1.0, records)
        if far_field:
            records, _, _ = _redistance_records(records, volume.shape, volume.resolution, volume.truncation, max_distance)
        self._set_records(volume._grid.voxels, volume._grid.resolution, records, records[:, 0].reshape(volume.shape) <= 0,
                          "TSDFField: no voxel of the volume is at or inside a surface (value <= 0)")
