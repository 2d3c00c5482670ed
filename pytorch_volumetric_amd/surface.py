"""Surface extraction: the level set of a sampled signed field as an indexed triangle mesh, by naive surface nets (include/pvamd.h
"Surface extraction", csrc/surface.hip) -- the arrow from a volume back to geometry.

The reference has no counterpart.  A TSDFVolume, an occupancy map taken through distance_transform, or any CachedSDF ends as
records on a lattice; extract_surface / CachedSDF.extract_mesh / TSDFVolume.extract_mesh hand the surface in them to everything
here that starts from a mesh: MeshObjectFactory(mesh=...), MeshSDF, sample_mesh_points, mesh_io.save_obj.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from pytorch_volumetric_amd import _lib, mesh_io
from pytorch_volumetric_amd._lattice import positive_finite, real

# include/pvamd.h "Surface extraction"; the cap on the voxels: vertex ids and quad counts in an int32
MIN_AXIS, MAX_AXIS, MAX_VOXELS = _lib.SURFACE_MIN_AXIS, _lib.LATTICE_MAX_AXIS, _lib.SURFACE_MAX_VOXELS


class Surface(NamedTuple):
    """extract_surface's result, every field on the GPU."""
    vertices: torch.Tensor           # (Nv, 3) float32, world coordinates
    faces: torch.Tensor              # (Nf, 3) int32 rows of vertex ids, counter-clockwise seen from the non-negative side
    normals: Optional[torch.Tensor]  # (Nv, 3) float32 unit normals interpolated from the gradients, None when not asked for

    def to_trimesh(self):
        """The mesh on the host as a mesh_io.TriMesh (float64 vertices, int64 faces): what MeshObjectFactory(mesh=...) and
        mesh_io.save_obj take."""
        return mesh_io.TriMesh(self.vertices.detach().cpu().numpy().astype(np.float64),
                               self.faces.detach().cpu().numpy().astype(np.int64))


def check_level(level):
    level = real("level", level)
    if not math.isfinite(level):
        raise ValueError(f"level must be finite, got {level}")
    return level


def check_normals(normals):
    if type(normals) is not bool:
        raise TypeError(f"normals must be a bool, got {type(normals).__name__}")
    return normals


def check_shape(shape, what="values"):
    """The lattice limits of the entry points, for the (nx, ny, nz) of `what`."""
    if min(shape) < MIN_AXIS or max(shape) > MAX_AXIS:
        raise ValueError(f"every axis of {what} must be in [{MIN_AXIS}, {MAX_AXIS}], got shape {tuple(shape)}")
    if shape[0] * shape[1] * shape[2] > MAX_VOXELS:
        raise ValueError(f"{what} must have at most 2^29 voxels, got shape {tuple(shape)}")


def _check_arguments(values, resolution, origin, level, gradients, valid):
    """The argument errors of extract_surface, raised before a GPU is asked for."""
    if not torch.is_tensor(values):
        values = torch.as_tensor(values)
    if values.is_complex():
        raise TypeError(f"values must have a real dtype, got {values.dtype}")
    if values.dim() != 3:
        raise ValueError(f"values must be a 3-D tensor, got shape {tuple(values.shape)}")
    check_shape(tuple(values.shape))
    resolution = positive_finite("resolution", resolution, strict=True)
    origin = tuple(origin)
    if len(origin) != 3:
        raise ValueError(f"origin must have three coordinates, got {len(origin)}")
    origin = tuple(real("origin", o) for o in origin)
    if not all(math.isfinite(o) for o in origin):
        raise ValueError(f"origin must be finite, got {origin}")
    level = check_level(level)
    if gradients is not None:
        if not torch.is_tensor(gradients):
            gradients = torch.as_tensor(gradients)
        if gradients.is_complex():
            raise TypeError(f"gradients must have a real dtype, got {gradients.dtype}")
        if tuple(gradients.shape) != tuple(values.shape) + (3,):
            raise ValueError(f"gradients must have shape {tuple(values.shape) + (3,)}, got {tuple(gradients.shape)}")
    if valid is not None:
        if not torch.is_tensor(valid):
            valid = torch.as_tensor(valid)
        if tuple(valid.shape) != tuple(values.shape):
            raise ValueError(f"valid must have shape {tuple(values.shape)}, got {tuple(valid.shape)}")
    return values, resolution, origin, level, gradients, valid


def lattice_desc(shape, resolution, origin):
    """A finalized pvamd_grid_t without storage whose voxel (0, 0, 0) is centred at `origin`: fmin = origin and fres = resolution
    as float32, which is all the surface kernels read of it."""
    from pytorch_volumetric_amd import voxel
    desc = _lib.GridDesc()
    for d in range(3):
        low, res = np.float32(origin[d]), np.float32(resolution)
        high = np.float32(low + np.float32(shape[d] - 1) * res)
        desc.fmin[d], desc.fmax[d], desc.fres[d] = float(low), float(high), float(res)
        desc.dmin[d], desc.dmax[d], desc.dres[d] = float(low), float(high), float(res)
        desc.shape[d] = shape[d]
    desc.index_f64 = 0
    desc.rule = voxel.INDEX_RULE
    desc.oob_mode = _lib.OOB_BOUNDING_BOX
    _lib.call("pvamd_grid_finalize", desc)
    return desc


def surface_of_records(desc, records, valid, level, want_normals):
    """pvamd_surface_count, one read of the two counts -- the only synchronisation -- and pvamd_surface_emit into tensors of that
    size, on the current stream.  records: contiguous float32 (n, 4) on the GPU; valid: contiguous uint8 (n,) there, or None."""
    dev = records.device
    nx, ny, nz = desc.shape
    with _lib.on_device(dev):
        scratch = _lib.scratch_buffer(_lib.surface_scratch_bytes(nx, ny, nz), dev)
        counts = torch.empty((2,), dtype=torch.int64, device=dev)
        _lib.call("pvamd_surface_count", desc, records, valid, level, scratch, counts)
        nv, nf = counts.tolist()
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((nv, 3), dtype=torch.float32, device=dev) if want_normals else None
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        if nv:
            _lib.call("pvamd_surface_emit", desc, records, valid, level, scratch, nv, nf, vertices, normals, faces)
    return Surface(vertices, faces, normals)


def extract_surface(values, resolution=1.0, origin=(0., 0., 0.), level=0.0, gradients=None, valid=None):
    """The surface `values == level` of a field sampled on a lattice as an indexed triangle mesh, in one fused count and one fused
    emit on the GPU (include/pvamd.h "Surface extraction"): naive surface nets.  Every lattice cell the surface passes through gets
    one vertex, at the mean of the crossings on the cell's edges (each placed by linear interpolation between its two samples);
    every lattice edge with a crossing gets a quad between the four cells round it, split into two triangles.  Vertices are shared:
    a closed surface away from the lattice's border comes out closed, and oriented with its normals toward increasing values.

    :param values: 3-D real tensor (nx, ny, nz), every axis MIN_AXIS to MAX_AXIS voxels and at most 2^29 in all: a signed field, for
        instance truncated.  NaN and infinite samples are unusable: a cell with one at a corner has no vertex.
    :param resolution: side length of a voxel
    :param origin: the centre of voxel (0, 0, 0)
    :param level: the value whose surface is wanted
    :param gradients: (nx, ny, nz, 3): the field's gradients at the samples; with them every vertex gets a unit normal
    :param valid: (nx, ny, nz), zero or False where a sample is not to be used (unseen space): nothing is meshed next to it
    :return: Surface(vertices, faces, normals) on the GPU; normals is None without gradients.  One synchronisation: the two
        counts are read to size the result.  A field without a crossing gives empty tensors, not an error.  The result carries no
        autograd graph.
    """
    values, resolution, origin, level, gradients, valid = _check_arguments(values, resolution, origin, level, gradients, valid)
    shape = tuple(values.shape)
    desc = lattice_desc(shape, resolution, origin)
    dev = values.device if values.is_cuda else _lib.require_gpu()
    records = torch.zeros(shape + (4,), dtype=torch.float32, device=dev)
    records[..., 0] = values.detach().to(device=dev)
    if gradients is not None:
        records[..., 1:] = gradients.detach().to(device=dev)
    if valid is not None:
        valid = (valid.detach().to(device=dev) != 0).to(torch.uint8).contiguous().reshape(-1)
    return surface_of_records(desc, records.reshape(-1, 4), valid, level, gradients is not None)
