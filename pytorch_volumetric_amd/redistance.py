"""Redistancing: the full Euclidean signed distance field of a sampled signed field, measured to its zero set at sub-voxel
precision (include/pvamd.h "Redistancing", csrc/redistance.hip) -- "ESDF from TSDF".

The reference has no counterpart.  A TSDFVolume's records are right next to the surface and truncated everywhere else; the
occupancy route (distance_transform) has the far field and a surface on voxel faces.  This takes the zero set from the first
and the reach from the second: TSDFVolume.to_sdf(far_field=True) is the consumer.
"""
import math
from typing import NamedTuple

import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd._lattice import positive, positive_finite, real

# include/pvamd.h "Redistancing"; the cap on the voxels: sites = flat index * 4 + axis in an int32
MIN_AXIS, MAX_AXIS, MAX_VOXELS = _lib.REDIST_MIN_AXIS, _lib.LATTICE_MAX_AXIS, _lib.REDIST_MAX_VOXELS


class Redistance(NamedTuple):
    """redistance's result, every field on the GPU and laid out like the values."""
    values: torch.Tensor     # (nx, ny, nz) float32, in units of `resolution`, with the sign of the input
    gradients: torch.Tensor  # (nx, ny, nz, 3) float32, unit length, toward increasing value
    sites: torch.Tensor      # (nx, ny, nz) int32: flat C-order index of the edge's lower voxel * 4 + the edge's axis; -1 without a
    #                          crossing in range, _lib.REDIST_KEPT inside the band
    squared: torch.Tensor    # (nx, ny, nz) float32 squared distance to the crossing in voxels; +inf where sites < 0


def _check_range(band, max_distance):
    """(band, max_distance) as floats: band >= 0, max_distance > 0 (inf: no limit), neither NaN."""
    band, max_distance = real("band", band), real("max_distance", max_distance)
    if not band >= 0:
        raise ValueError(f"band must be zero or positive, got {band}")
    return band, positive("max_distance", max_distance)


def _check_arguments(values, resolution, band, gradients, max_distance):
    """The argument errors of redistance, raised before a GPU is asked for."""
    if not torch.is_tensor(values):
        values = torch.as_tensor(values)
    if values.is_complex():
        raise TypeError(f"values must have a real dtype, got {values.dtype}")
    if values.dim() != 3:
        raise ValueError(f"values must be a 3-D tensor, got shape {tuple(values.shape)}")
    if min(values.shape) < MIN_AXIS or max(values.shape) > MAX_AXIS:
        raise ValueError(f"every axis of values must be in [{MIN_AXIS}, {MAX_AXIS}], got shape {tuple(values.shape)}")
    if values.numel() > MAX_VOXELS:
        raise ValueError(f"values must have at most 2^29 voxels, got shape {tuple(values.shape)}")
    resolution = positive_finite("resolution", resolution, strict=True)
    band, max_distance = _check_range(band, max_distance)
    if gradients is not None:
        if not torch.is_tensor(gradients):
            gradients = torch.as_tensor(gradients)
        if gradients.is_complex():
            raise TypeError(f"gradients must have a real dtype, got {gradients.dtype}")
        if tuple(gradients.shape) != tuple(values.shape) + (3,):
            raise ValueError(f"gradients must have shape {tuple(values.shape) + (3,)}, got {tuple(gradients.shape)}")
    elif band > 0:
        raise ValueError("band > 0 keeps the records of the voxels inside it: their gradients must be given")
    return values, resolution, band, gradients, max_distance


def _redistance_records(records, shape, resolution, band, max_distance):
    """One pvamd_redistance call on the current stream over contiguous float32 (n, 4) records on the GPU: (records (n, 4),
    sites (n,), squared (n,)).  Nothing comes back to the host."""
    dev = records.device
    nx, ny, nz = shape
    n = records.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sites = torch.empty((n,), dtype=torch.int32, device=dev)
    squared = torch.empty((n,), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch_buffer(_lib.redistance_scratch_bytes(nx, ny, nz), dev)
        _lib.call("pvamd_redistance", records, nx, ny, nz, resolution, band, max_distance, out, sites, squared, scratch)
    return out, sites, squared


def redistance(values, resolution=1.0, band=0.0, gradients=None, max_distance=math.inf):
    """The Euclidean signed distance from every voxel to the zero set of a sampled signed field, in one fused call on the GPU
    (include/pvamd.h "Redistancing").  The zero set is where the samples change sign along the lattice edges, placed by linear
    interpolation between the two samples; the result keeps each voxel's sign.

    :param values: 3-D real tensor (nx, ny, nz), every axis MIN_AXIS to MAX_AXIS voxels: a signed field, for instance truncated.  Only the
        signs and the ratios across sign changes matter.  NaN and infinite samples give their edges no crossing.
    :param resolution: side length of a voxel; the values returned are in its units
    :param band: voxels with |value| < band keep their value and gradient as they are (a TSDF's band round the surface)
    :param gradients: (nx, ny, nz, 3), needed when band > 0: the gradients of the kept voxels
    :param max_distance: voxels further than this from every crossing get +/-max_distance and a zero gradient.  It also bounds
        the work: without it a scan through space without crossings runs the length of the grid.
    :return: Redistance(values, gradients, sites, squared).  Nothing synchronises with the host: a field without any sign change
        gives +/-max_distance everywhere rather than an error.  The result carries no autograd graph.
    """
    values, resolution, band, gradients, max_distance = _check_arguments(values, resolution, band, gradients, max_distance)
    shape = tuple(values.shape)
    dev = values.device if values.is_cuda else _lib.require_gpu()
    records = torch.zeros(shape + (4,), dtype=torch.float32, device=dev)
    records[..., 0] = values.detach().to(device=dev)
    if gradients is not None:
        records[..., 1:] = gradients.detach().to(device=dev)
    out, sites, squared = _redistance_records(records.reshape(-1, 4), shape, resolution, band, max_distance)
    return Redistance(out[:, 0].reshape(shape), out[:, 1:4].reshape(*shape, 3), sites.reshape(shape), squared.reshape(shape))
