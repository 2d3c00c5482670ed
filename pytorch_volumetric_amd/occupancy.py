"""Signed distance fields from voxel occupancy: the fused Euclidean distance transform (include/pvamd.h "Distance transform",
csrc/distance_transform.hip) and the ObjectFrameSDF over a VoxelGrid that it fills.

The reference has no counterpart: its VoxelGrid / ExpandingVoxelGrid hold what a sensor saw (voxel.py:42-103) and every SDF it
can query starts from a mesh or a closed form.  With this producer an observed scene is a leaf like any mesh cache.
"""
from typing import NamedTuple

import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd._lattice import positive_finite
from pytorch_volumetric_amd.sdf import CachedSDF, ObjectFrameSDF, _restore
from pytorch_volumetric_amd.voxel import RangeView

# include/pvamd.h "Distance transform"
MIN_AXIS, MAX_AXIS, MAX_VOXELS = _lib.EDT_MIN_AXIS, _lib.LATTICE_MAX_AXIS, _lib.EDT_MAX_VOXELS


class DistanceTransform(NamedTuple):
    """distance_transform's result, every field on the GPU and laid out like the occupancy."""
    values: torch.Tensor     # (nx, ny, nz) float32, in units of `resolution`
    gradients: torch.Tensor  # (nx, ny, nz, 3) float32, toward increasing value
    sites: torch.Tensor      # (nx, ny, nz) int32 flat C-order index of the nearest site, -1 without one
    squared: torch.Tensor    # (nx, ny, nz) int32 squared distance to it in voxels, _lib.EDT_NO_SITE without one


def _check_arguments(occupied, resolution, signed):
    """The argument errors of distance_transform, raised before a GPU is asked for."""
    if type(signed) is not bool:
        raise TypeError(f"signed must be a bool, got {type(signed).__name__}")
    if not torch.is_tensor(occupied):
        occupied = torch.as_tensor(occupied)
    if occupied.dim() != 3:
        raise ValueError(f"occupied must be a 3-D tensor, got shape {tuple(occupied.shape)}")
    if min(occupied.shape) < MIN_AXIS or max(occupied.shape) > MAX_AXIS:
        raise ValueError(f"every axis of occupied must be in [{MIN_AXIS}, {MAX_AXIS}], got shape {tuple(occupied.shape)}")
    if occupied.numel() > MAX_VOXELS:
        raise ValueError(f"occupied must have at most 2^31 - 1 voxels, got shape {tuple(occupied.shape)}")
    return occupied, positive_finite("resolution", resolution)


def _transform(occupied, resolution, signed):
    """One pvamd_distance_transform call on the current stream: (occupancy bytes, records (n, 4), sites (n,), squared (n,)) on the
    GPU.  Nothing comes back to the host."""
    dev = occupied.device if occupied.is_cuda else _lib.require_gpu()
    occ = occupied.detach().to(device=dev)
    if occ.dtype != torch.uint8:
        occ = (occ if occ.dtype == torch.bool else occ != 0).view(torch.uint8)
    occ = occ.contiguous()
    nx, ny, nz = occ.shape
    n = occ.numel()
    records = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sites = torch.empty((n,), dtype=torch.int32, device=dev)
    squared = torch.empty((n,), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch_buffer(_lib.distance_transform_scratch_bytes(nx, ny, nz, signed), dev)
        _lib.call("pvamd_distance_transform", occ, nx, ny, nz, resolution, signed, records, sites, squared, scratch)
    return occ, records, sites, squared


def distance_transform(occupied, resolution=1.0, signed=True):
    """The exact Euclidean distance transform of a voxel occupancy grid with its gradient, in one fused call on the GPU
    (include/pvamd.h "Distance transform").

    :param occupied: 3-D bool, uint8 or numeric tensor (nx, ny, nz), non-zero = occupied; moved to the GPU like other inputs
    :param resolution: side length of a voxel; values are in its units
    :param signed: True: a free voxel gets the distance to the nearest occupied voxel minus half a voxel, an occupied one the
        negated distance to the nearest free voxel plus half a voxel -- the surface lies on the voxel faces.  False: the distance
        to the nearest occupied voxel, zero on occupied voxels.
    :return: DistanceTransform(values, gradients, sites, squared).  Among equally near sites the one with the smallest flat index
        is reported, and the gradient points away from it (toward it for an occupied voxel).  Nothing synchronises with the host:
        a grid without occupied voxels (signed: also one without free voxels) gives +inf / -inf values, zero gradients, sites of
        -1 and squared of 2^31 - 1 rather than an error.  The result carries no autograd graph.
    """
    occupied, resolution = _check_arguments(occupied, resolution, signed)
    shape = tuple(occupied.shape)
    _, records, sites, squared = _transform(occupied, resolution, signed)
    return DistanceTransform(records[:, 0].reshape(shape), records[:, 1:4].reshape(*shape, 3), sites.reshape(shape),
                             squared.reshape(shape))


class OccupancySDF(ObjectFrameSDF):
    """The SDF of the occupied voxels of a 3-D VoxelGrid / ExpandingVoxelGrid: distance_transform over the grid's own lattice, run
    once at construction, then answered like a nearest-mode BOUNDING_BOX CachedSDF over that lattice (the same kernels and
    descriptor: pvamd_cached_query / pvamd_cached_query_f64).  A snapshot: later writes to the grid do not reach it."""

    def __init__(self, voxels, signed=True, threshold=None):
        """
        :param voxels: a 3-D VoxelGrid or ExpandingVoxelGrid; its resolution, range_per_dim and shape are the lattice
        :param signed: as for distance_transform
        :param threshold: None: a voxel is occupied when its value is != 0; a number: when its value is > threshold
        """
        if type(signed) is not bool:
            raise TypeError(f"signed must be a bool, got {type(signed).__name__}")
        data = voxels.get_voxel_values()
        if data.dim() != 3 or min(data.shape) < 2:
            raise ValueError(f"OccupancySDF needs a 3-D voxel grid with at least two voxels per axis, got shape {tuple(data.shape)}")
        occupied, resolution = _check_arguments(data != 0 if threshold is None else data > threshold, voxels.resolution, signed)
        self.signed = signed
        occ, records, self._sites, self._squared = _transform(occupied, resolution, signed)
        count = self._set_records(voxels.voxels, voxels.resolution, records, occ, "OccupancySDF: the grid has no occupied voxel")
        if signed and count == occ.numel():
            raise ValueError("OccupancySDF: signed=True needs at least one free voxel, every voxel of the grid is occupied")

    def _set_records(self, view, resolution, records, inside, empty):
        """What every producer of lattice records ends its __init__ with: the lattice of `view` (a grid's ValueRangeView: ranges,
        shape, rule), the (n, 4) records over it, and the box of the voxels `inside` (a mask shaped like the lattice) marks as at
        or inside the surface.  Returns how many those are; none is a ValueError(empty)."""
        self.resolution = resolution
        self.ranges = list(view._ranges)  # the element types decide the dtype of the index arithmetic (voxel.RangeView)
        self._view = RangeView(self.ranges, view.shape, rule=view._rule)
        self._records = records
        # the one synchronisation: how many voxels are inside and which index box they fill
        index = inside.nonzero()
        if index.shape[0] == 0:
            raise ValueError(empty)
        lo, hi = index.amin(dim=0).cpu().double(), index.amax(dim=0).cpu().double()
        half = self._view.dres / 2
        self._box = torch.stack((self._view.dmin + lo * self._view.dres - half, self._view.dmin + hi * self._view.dres + half), dim=1)
        self._desc = None
        return index.shape[0]

    def same_lattice(self, resolution, range_per_dim, shape):
        """Whether a grid of `shape` voxels of `resolution` over `range_per_dim` has this field's voxel centres, in the same index
        dtype: what lets a CachedSDF take the records as they are."""
        if tuple(int(s) for s in shape) != self._view.shape or len(range_per_dim) != 3 or resolution != self.resolution:
            return False
        other = RangeView(range_per_dim, shape, rule=self._view.rule)
        return other.index_f64 == self._view.index_f64 and torch.equal(other.min, self._view.min) and \
            torch.equal(other.max, self._view.max) and torch.equal(other.resolution, self._view.resolution)

    def surface_bounding_box(self, padding=0., padding_ratio=0.):
        """(3, 2) float64: the box of the occupied voxel cubes (centres -/+ half a voxel), inflated like ObjectFactory.bounding_box."""
        box = self._box.clone()
        extents = box[:, 1] - box[:, 0]
        box[:, 0] -= padding + padding_ratio * extents
        box[:, 1] += padding + padding_ratio * extents
        return box

    def _grid_desc(self):
        """pvamd_grid_t over the records: CachedSDF._grid_desc's statements for the BOUNDING_BOX strategy."""
        if self._desc is None:
            desc = _lib.GridDesc()
            desc.vox = self._records.data_ptr()
            self._view.fill(desc)
            bb = self._box.to(dtype=torch.float32)
            for d in range(3):
                desc.bb_min[d], desc.bb_max[d] = bb[d, 0].item(), bb[d, 1].item()
                desc.dbb_min[d], desc.dbb_max[d] = self._box[d, 0].item(), self._box[d, 1].item()
            desc.oob_mode = _lib.OOB_BOUNDING_BOX
            _lib.call("pvamd_grid_finalize", desc)
            self._desc = desc
        return self._desc

    def __call__(self, points_in_object_frame):
        """(values, gradients) at (..., 3) points in the caller's dtype on the caller's device: the record of the nearest voxel in
        range, the distance to surface_bounding_box() outside.  float64 points are looked up in float64.  No autograd graph."""
        flat, lead, dtype, device = _lib.as_query_points(points_in_object_frame, self._records.device, keep_f64=True)
        P = flat.shape[0]
        val = torch.empty((P,), dtype=flat.dtype, device=flat.device)
        grad = torch.empty((P, 3), dtype=flat.dtype, device=flat.device)
        with _lib.on_device(flat.device):
            _lib.call("pvamd_cached_query", self._grid_desc(), flat, P, val, grad, None, f64=flat.dtype == torch.float64)
        return _restore(val, lead, (), dtype, device), _restore(grad, lead, (3,), dtype, device)


def cached_sdf_from_voxels(name, voxels, signed=True, threshold=None, device="cuda", interpolation="nearest"):
    """A CachedSDF of the occupied voxels of a 3-D VoxelGrid / ExpandingVoxelGrid over the grid's own lattice: the records of
    OccupancySDF(voxels, signed, threshold), taken as they are and not written to a cache file.  Ray-cast it, refine a pose
    against it or compose it like any mesh cache."""
    field = OccupancySDF(voxels, signed=signed, threshold=threshold)
    return CachedSDF(name, field.resolution, field.ranges, field, device=device, cache_path=None, interpolation=interpolation)
