"""What the volume modules (occupancy, occupancy_map, tsdf, redistance) share before any GPU is asked for: their argument checks
and the lattice a volume is built over (include/pvamd.h "Volume lattices")."""
import math
import numbers

import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd.voxel import get_divisible_range_by_resolution
from pytorch_volumetric_amd.voxel_containers import VoxelGrid


def real(name, value):
    """value as a float; a bool, or anything that is not a real number, is a TypeError."""
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise TypeError(f"{name} must be a real number, got {type(value).__name__}")
    return float(value)


def positive_finite(name, value, strict=False):
    """strict: value must pass real(); else whatever float() takes."""
    value = real(name, value) if strict else float(value)
    if not (math.isfinite(value) and value > 0):
        raise ValueError(f"{name} must be finite and positive, got {value}")
    return value


def positive(name, value):
    """Positive, +inf allowed (no limit), NaN refused."""
    value = float(value)
    if not value > 0:
        raise ValueError(f"{name} must be positive (inf: no limit), got {value}")
    return value


def lattice_grid(resolution, range_per_dim, what, min_axis, device):
    """The opening of a volume's constructor: the float32 VoxelGrid(resolution, range_per_dim) on `device` ("meta": a shape and a
    descriptor without storage) whose lattice the volume lives on, its resolution a float.  `what` names the volume in the
    messages ("an OccupancyMap").  A GPU is asked for only after every check, and only for a grid on one."""
    resolution = positive_finite("resolution", resolution)
    if len(range_per_dim) != 3:
        raise ValueError(f"{what} is 3-D: range_per_dim needs three (low, high) pairs, got {len(range_per_dim)}")
    cells = [round((high - low) / resolution) + 1 for low, high in get_divisible_range_by_resolution(resolution, range_per_dim)]
    if min(cells) < min_axis or max(cells) > _lib.LATTICE_MAX_AXIS:
        raise ValueError(f"every axis of {what} must have {min_axis} to {_lib.LATTICE_MAX_AXIS} voxels, got {tuple(cells)}")
    device = torch.device(device)
    if device.type == "cuda":
        _lib.require_gpu()
    return VoxelGrid(resolution, range_per_dim, dtype=torch.float32, device=device)
