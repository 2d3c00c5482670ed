"""Occupancy mapping from sensor rays: a log-odds map over a VoxelGrid's lattice that every scan both adds to and carves
(include/pvamd.h "Ray integration", csrc/ray_integrate.hip).

The reference has no counterpart: its containers are written with grid[points] = value (voxel.py:97-103), which can only add, so a
voxel a sensor once reported stays occupied and free space is never told from space nobody looked at.  An OccupancyMap is what
turns depth images into the occupancy that distance_transform / cached_sdf_from_voxels make a CachedSDF of.
"""
import math

import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd._lattice import lattice_grid, positive, real
from pytorch_volumetric_amd.occupancy import cached_sdf_from_voxels
from pytorch_volumetric_amd.voxel_containers import VoxelGrid

MIN_AXIS, MAX_AXIS = _lib.RAY_MARK_MIN_AXIS, _lib.LATTICE_MAX_AXIS  # include/pvamd.h "Ray integration"
UNKNOWN = ("free", "occupied")


def _log_odds(p):
    return math.log(p / (1.0 - p))


def _check_unknown(unknown):
    if unknown not in UNKNOWN:
        raise ValueError(f"unknown must be one of {UNKNOWN}, got {unknown!r}")


def _check_rays(origins, endpoints, max_range):
    """The argument errors of a scan, raised before a GPU is asked for: (origins, endpoints, max_range, shape of the scan)."""
    origins = origins if torch.is_tensor(origins) else torch.as_tensor(origins)
    endpoints = endpoints if torch.is_tensor(endpoints) else torch.as_tensor(endpoints)
    for name, t in (("origins", origins), ("endpoints", endpoints)):
        if t.dim() < 1 or t.shape[-1] != 3:
            raise ValueError(f"{name} must have last dimension 3, got {tuple(t.shape)}")
    try:
        lead = torch.broadcast_shapes(origins.shape[:-1], endpoints.shape[:-1])
    except RuntimeError as e:
        raise ValueError(f"origins {tuple(origins.shape)} and endpoints {tuple(endpoints.shape)} do not broadcast") from e
    return origins, endpoints, positive("max_range", max_range), lead


class OccupancyMap:
    """A log-odds occupancy map over the lattice of a float32 VoxelGrid(resolution, range_per_dim).

    integrate() takes one scan: the voxels the rays cross lose log-odds, the voxels their endpoints fall into gain them, each once
    per scan however many rays agree, a hit taking precedence over any number of crossings.  The endpoint's voxel is the one
    grid[endpoint] = 1 writes on a VoxelGrid over the same range.  Everything stays on the GPU and nothing carries an autograd graph.
    """

    def __init__(self, resolution, range_per_dim, device="cuda", prob_hit=0.7, prob_miss=0.4, clamp=(0.12, 0.97)):
        """
        :param resolution: side length of a voxel
        :param range_per_dim: three (low, high) pairs, snapped to whole voxels like a VoxelGrid's; the range is fixed, parts of a
            ray outside it are clipped
        :param prob_hit: probability a voxel holding an endpoint is given by that scan, in (0.5, 1)
        :param prob_miss: probability a voxel crossed by a ray is given, in (0, 0.5)
        :param clamp: (lo, hi) probabilities, 0 < lo < 0.5 < hi < 1, that the map never leaves: what bounds the number of scans
            it takes to change its mind
        """
        prob_hit, prob_miss = float(prob_hit), float(prob_miss)
        if not 0.5 < prob_hit < 1.0:
            raise ValueError(f"prob_hit must be in (0.5, 1), got {prob_hit}")
        if not 0.0 < prob_miss < 0.5:
            raise ValueError(f"prob_miss must be in (0, 0.5), got {prob_miss}")
        lo, hi = (float(c) for c in clamp)
        if not 0.0 < lo < 0.5 < hi < 1.0:
            raise ValueError(f"clamp must be 0 < lo < 0.5 < hi < 1, got {(lo, hi)}")
        # float64 log, rounded to float32 once: the four numbers the update kernel is handed
        self.l_hit, self.l_miss, self.l_min, self.l_max = (
            torch.tensor(_log_odds(p), dtype=torch.float64).to(torch.float32).item() for p in (prob_hit, prob_miss, lo, hi))
        self._grid = lattice_grid(resolution, range_per_dim, "an OccupancyMap", MIN_AXIS, device)
        self.resolution, self.range_per_dim, self.device = self._grid.resolution, range_per_dim, self._grid.device
        shape = tuple(self._grid.get_voxel_values().shape)
        self._observed = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        self._marks = torch.zeros(shape, dtype=torch.uint8, device=self.device)  # zero between scans: the update clears it

    @property
    def log_odds(self):
        """(nx, ny, nz) float32: the map's storage.  +0.0 where no scan touched."""
        return self._grid.get_voxel_values()

    @property
    def observed(self):
        """(nx, ny, nz) bool: whether some scan crossed or hit the voxel."""
        return self._observed.view(torch.bool)

    @property
    def shape(self):
        return tuple(self.log_odds.shape)

    def probability(self):
        """(nx, ny, nz) float32: 1 / (1 + exp(-log_odds)); 0.5 where nothing was observed."""
        return torch.sigmoid(self.log_odds)

    def occupied(self, threshold=0.5, unknown="free"):
        """(nx, ny, nz) bool: the observed voxels whose probability exceeds `threshold`; with unknown="occupied" also every
        voxel no scan has touched (what a planner that must not enter unseen space wants)."""
        _check_unknown(unknown)
        threshold = real("threshold", threshold)
        level = -math.inf if threshold <= 0 else (math.inf if threshold >= 1 else _log_odds(threshold))
        seen = self.observed
        occupied = (self.log_odds > level) & seen
        return occupied | ~seen if unknown == "occupied" else occupied

    def reset(self):
        """Forget every scan."""
        self.log_odds.zero_()
        self._observed.zero_()
        self._marks.zero_()

    def _mark(self, origins, endpoints, max_range, marks):
        """One pvamd_ray_mark call on the current stream; False when the scan holds no ray."""
        origins, endpoints, max_range, lead = _check_rays(origins, endpoints, max_range)
        if math.prod(lead) == 0:
            return False
        if self.device.type != "cuda":
            raise _lib.PvamdError(f"ray integration runs on the GPU and this map lives on {self.device}; there is no CPU fallback")
        shared = origins.numel() == 3  # one eye for the whole scan: handed over as it is, not expanded
        endpoints = endpoints.detach().to(device=self.device, dtype=torch.float32).expand(*lead, 3).reshape(-1, 3).contiguous()
        origins = origins.detach().to(device=self.device, dtype=torch.float32)
        origins = (origins.reshape(1, 3) if shared else origins.expand(*lead, 3).reshape(-1, 3)).contiguous()
        R = endpoints.shape[0]
        with _lib.on_device(self.device):
            _lib.call("pvamd_ray_mark", self._grid.voxels._grid_desc(), origins, shared, endpoints, R, max_range, marks)
        return True

    def integrate(self, origins, endpoints, max_range=math.inf):
        """One scan: rays from `origins` ((3,) for one eye, or (..., 3)) to `endpoints` (..., 3), broadcast against each other.
        A ray longer than `max_range` carves up to that range and reports no hit; a ray with a non-finite coordinate is ignored.
        Two launches to classify the voxels and one to move the map; nothing comes back to the host.  No rays: a no-op."""
        if not self._mark(origins, endpoints, max_range, self._marks):
            return
        with _lib.on_device(self.device):
            _lib.call("pvamd_occupancy_update", self._marks, self._marks.numel(), self.l_hit, self.l_miss, self.l_min, self.l_max,
                      self.log_odds, self._observed)

    def to_sdf(self, name, signed=True, unknown="free", interpolation="nearest", threshold=0.5):
        """A CachedSDF of occupied(threshold, unknown) over the map's lattice (cached_sdf_from_voxels): a snapshot that can be
        ray-cast, composed with a robot or used for pose refinement like any mesh cache."""
        occupied = self.occupied(threshold=threshold, unknown=unknown)
        voxels = VoxelGrid(self.resolution, self.range_per_dim, dtype=torch.bool, device=self.device)
        voxels.get_voxel_values().copy_(occupied)
        return cached_sdf_from_voxels(name, voxels, signed=signed, device=self.device, interpolation=interpolation)


def ray_marks(omap, origins, endpoints, max_range=math.inf):
    """(nx, ny, nz) uint8 on the GPU: how one scan classifies the voxels of `omap`'s lattice -- _lib.MARK_HIT where an endpoint
    falls, _lib.MARK_FREE where only rays passed, 0 elsewhere.  The map is not touched."""
    marks = torch.zeros(omap.shape, dtype=torch.uint8, device=omap.device)
    omap._mark(origins, endpoints, max_range, marks)
    return marks
