"""ObjectFrameSDF family over the HIP engine: MeshSDF, CachedSDF, ComposedSDF, SphereSDF and the ObjectFactory
they hang off.  Same names, signatures, output shapes and error behaviour as pytorch_volumetric/sdf.py (reference
lines cited per member); every `__call__` is one (or, for uncached leaves, a few) kernel launch through
libpvamd.so instead of the reference's torch-op sequences and Embree round trips.
"""
import abc
import ctypes
import enum
import logging
import math
import numbers
import os
import typing
from functools import partial
from typing import NamedTuple, Union

import numpy as np
import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import mesh_io
from pytorch_volumetric_amd import transforms as tf
from pytorch_volumetric_amd.voxel import (RangeView, get_coordinates_and_points_in_grid,
                                          get_divisible_range_by_resolution)

logger = logging.getLogger(__name__)


class SDFQuery(NamedTuple):
    """sdf.py:23-27"""
    closest: torch.Tensor
    distance: torch.Tensor
    gradient: torch.Tensor
    normal: Union[torch.Tensor, None]



class MinOverPoints(NamedTuple):
    """ComposedSDF.min_over_points / RobotSDF.min_over_points: per pair, the smallest point index that minimises the value, and
    the value and gradient there (include/pvamd.h "Minimum over points")."""
    values: torch.Tensor
    indices: torch.Tensor
    gradients: torch.Tensor


class RayCast(NamedTuple):
    """CachedSDF.ray_cast / ComposedSDF.ray_cast / RobotSDF.ray_cast: per ray the parameter t of the last evaluated point
    o + t d, why the march stopped (RAY_MISS / RAY_HIT / RAY_MAX_STEPS / RAY_INVALID, uint8), the value and gradient read there
    and the number of evaluations (int32) (include/pvamd.h "Ray casting")."""
    t: torch.Tensor
    status: torch.Tensor
    values: torch.Tensor
    gradients: torch.Tensor
    steps: torch.Tensor


RAY_MISS, RAY_HIT, RAY_MAX_STEPS, RAY_INVALID = _lib.RAY_MISS, _lib.RAY_HIT, _lib.RAY_MAX_STEPS, _lib.RAY_INVALID


class MeshRayHits(NamedTuple):
    """ObjectFactory.cast_rays: per ray the parameter t of the first triangle hit on o + t d (inf: none), that triangle's
    original face id (int64, -1: none), its stored unit face normal (not flipped towards the ray) and the barycentrics (u, v) of
    the hit, (1 - u - v) a + u b + v c on the face's corners; zeros on a miss (include/pvamd.h "Mesh ray casting")."""
    t: torch.Tensor
    face_ids: torch.Tensor
    normals: torch.Tensor
    uv: torch.Tensor


def _ray_window(t_min, t_max):
    """(t_min, t_max) of a mesh ray cast as floats, or the error include/pvamd.h "Mesh ray casting" asks for."""
    for name, x in (("t_min", t_min), ("t_max", t_max)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real):
            raise TypeError(f"{name} must be a Python real number, got {type(x).__name__}")
    if math.isnan(t_min) or math.isnan(t_max):
        raise ValueError(f"t_min and t_max must not be NaN, got {t_min!r} and {t_max!r}")
    return float(t_min), float(t_max)


class HingeOverPoints(NamedTuple):
    """ComposedSDF.hinge_over_points / RobotSDF.hinge_over_points: per pair, sum over points of max(margin - v, 0) ** power and
    the number of points with v < margin (include/pvamd.h "Hinge penalty over points")."""
    values: torch.Tensor
    counts: torch.Tensor


class LeafPairHinge(NamedTuple):
    """ComposedSDF.leaf_pair_hinge / RobotSDF.self_collision_hinge: per configuration and ordered leaf pair (s, t), the sum over
    leaf t's points of max(margin - v, 0) ** power under leaf s's SDF and the number of those points with v < margin
    (include/pvamd.h "Leaf-pair hinge")."""
    values: torch.Tensor
    counts: torch.Tensor


class LeafPairDistance(NamedTuple):
    """ComposedSDF.leaf_pair_distance / RobotSDF.self_collision_distance: per configuration and ordered leaf pair (s, t), the point
    of leaf t's set where leaf s's SDF is smallest, the value there and leaf s's gradient expressed in leaf t's frame
    (include/pvamd.h "Leaf-pair distance")."""
    values: torch.Tensor
    indices: torch.Tensor
    gradients: torch.Tensor


def _hinge_args(margin, power):
    """margin: a finite Python real (rounded to the query dtype by the caller); power: 1 or 2."""
    if isinstance(margin, bool) or not isinstance(margin, numbers.Real):
        raise TypeError(f"margin must be a Python real number, got {type(margin).__name__}")
    margin = float(margin)
    if not math.isfinite(margin):
        raise ValueError(f"margin must be finite, got {margin!r}")
    if isinstance(power, bool) or power not in (1, 2):
        raise ValueError(f"power must be 1 or 2, got {power!r}")
    return margin, int(power)


def _ray_args(t_min, t_max, hit_tolerance, step_scale, max_steps):
    """The five scalars of a ray cast as (float, float, float, float, int), or the error include/pvamd.h "Ray casting" asks for;
    the caller rounds the reals once to the query dtype."""
    reals = {"t_min": t_min, "t_max": t_max, "hit_tolerance": hit_tolerance, "step_scale": step_scale}
    for name, x in reals.items():
        if isinstance(x, bool) or not isinstance(x, numbers.Real):
            raise TypeError(f"{name} must be a Python real number, got {type(x).__name__}")
        reals[name] = float(x)
    if isinstance(max_steps, bool) or not isinstance(max_steps, numbers.Integral):
        raise TypeError(f"max_steps must be an integer, got {type(max_steps).__name__}")
    if math.isnan(reals["t_min"]) or math.isnan(reals["t_max"]):
        raise ValueError(f"t_min and t_max must not be NaN, got {t_min!r} and {t_max!r}")
    if not (math.isfinite(reals["hit_tolerance"]) and reals["hit_tolerance"] >= 0):
        raise ValueError(f"hit_tolerance must be finite and >= 0, got {hit_tolerance!r}")
    if not (math.isfinite(reals["step_scale"]) and reals["step_scale"] > 0):
        raise ValueError(f"step_scale must be finite and > 0, got {step_scale!r}")
    if not 1 <= max_steps <= 65535:
        raise ValueError(f"max_steps must lie in [1, 65535], got {max_steps!r}")
    return reals["t_min"], reals["t_max"], reals["hit_tolerance"], reals["step_scale"], int(max_steps)


def _ray_inputs(origins, directions):
    """(origins, directions) broadcast against each other -> (origins, directions, lead, dtype): both detached, of the broadcast
    shape lead + (3,) (views, not yet contiguous) and of one floating dtype (an integer dtype counts as float32, as for points)."""
    if not torch.is_tensor(origins):
        origins = torch.as_tensor(origins)
    if not torch.is_tensor(directions):
        directions = torch.as_tensor(directions)
    for name, x in (("origins", origins), ("directions", directions)):
        if x.dim() < 1 or x.shape[-1] != 3:
            raise ValueError(f"ray {name} must have last dimension 3, got {tuple(x.shape)}")
    try:
        shape = torch.broadcast_shapes(origins.shape, directions.shape)
    except RuntimeError as e:
        raise ValueError(f"ray origins {tuple(origins.shape)} and directions {tuple(directions.shape)} do not broadcast") from e
    dtype = torch.promote_types(origins.dtype, directions.dtype)
    if not dtype.is_floating_point:
        dtype = torch.float32
    return origins.detach().expand(shape), directions.detach().expand(shape), tuple(shape[:-1]), dtype


def _ray_graph(differentiable, origins, directions, lead, tf_grad=False):
    """Whether a ray cast keeps an autograd graph (include/pvamd.h "Ray casting: gradient of the hit distance"): None -- today's
    path -- unless differentiable is True, grad mode is on and the origins, the directions or (tf_grad) a composition's
    transforms require grad; else (origins, directions) expanded to the rays' shape lead + (3,), still attached."""
    if not isinstance(differentiable, bool):
        raise TypeError(f"differentiable must be True or False, got {differentiable!r}")
    if not (differentiable and torch.is_grad_enabled()):
        return None
    origins = origins if torch.is_tensor(origins) else torch.as_tensor(origins)
    directions = directions if torch.is_tensor(directions) else torch.as_tensor(directions)
    if not (origins.requires_grad or directions.requires_grad or tf_grad):
        return None
    return origins.expand(*lead, 3), directions.expand(*lead, 3)


def _ray_outputs(shape, dtype, dev):
    """(t, status, values, gradients, steps) buffers of the ray-cast entry points, in the C ABI's argument order."""
    return (torch.empty(shape, dtype=dtype, device=dev), torch.empty(shape, dtype=torch.uint8, device=dev),
            torch.empty(shape, dtype=dtype, device=dev), torch.empty((*shape, 3), dtype=dtype, device=dev),
            torch.empty(shape, dtype=torch.int32, device=dev))


def _ray_result(out, shape, device):
    t, status, val, grad, steps = out
    return RayCast(t.reshape(shape).to(device), status.reshape(shape).to(device), val.reshape(shape).to(device),
                   grad.reshape(*shape, 3).to(device), steps.reshape(shape).to(device))


def _ray_march(sdf, o, d, t_min, t_max, eps, step_scale, max_steps):
    """The loop of include/pvamd.h "Ray casting" in torch around sdf(points) for (R, 3) rays of one dtype on one device: every
    step queries all the rays and torch.where keeps the finished ones as they were.  Stops early (one device -> host
    synchronisation per step) when no ray is left marching.  Returns the five (R,) / (R, 3) results."""
    R, dtype, dev = o.shape[0], o.dtype, o.device
    t_max, eps, step_scale = (torch.tensor(x, dtype=dtype, device=dev) for x in (t_max, eps, step_scale))
    t = torch.full((R,), t_min, dtype=dtype, device=dev)
    t_read = t  # the parameter of each ray's last evaluated point: what is reported (after max_steps, t itself has moved on)
    v = torch.full((R,), math.nan, dtype=dtype, device=dev)
    g = torch.full((R, 3), math.nan, dtype=dtype, device=dev)
    steps = torch.zeros((R,), dtype=torch.int32, device=dev)
    active = t <= t_max
    status = torch.where(active, RAY_MAX_STEPS, RAY_MISS).to(torch.uint8)
    for _ in range(max_steps):
        if not bool(active.any()):
            break
        vv, gg = sdf(o + t.unsqueeze(-1) * d)
        vv, gg = vv.reshape(R).to(device=dev, dtype=dtype), gg.reshape(R, 3).to(device=dev, dtype=dtype)
        v, g, t_read = torch.where(active, vv, v), torch.where(active.unsqueeze(-1), gg, g), torch.where(active, t, t_read)
        steps = steps + active.to(torch.int32)
        nan = vv != vv
        hit = ~nan & (vv <= eps)
        tn = t + step_scale * vv
        miss = ~nan & ~hit & ~(tn <= t_max)
        go = active & ~nan & ~hit & ~miss
        for code, stop in ((RAY_INVALID, nan), (RAY_HIT, hit), (RAY_MISS, miss)):
            status = torch.where(active & stop, torch.tensor(code, dtype=torch.uint8, device=dev), status)
        t = torch.where(go, tn, t)
        active = go
    return t_read, status, v, g, steps


def first_argmin(v):
    """The index rule of min_over_points along the last dimension: a NaN counts as the minimum, -0.0 and +0.0 tie, and the
    smallest index among the minima wins.  Plain torch, no device -> host synchronisation."""
    nan = torch.isnan(v)
    hit = torch.where(nan.any(dim=-1, keepdim=True), nan, v == v.amin(dim=-1, keepdim=True))
    return hit.to(torch.uint8).argmax(dim=-1)  # argmax returns the first of equal maxima

def _restore(t, lead, tail, dtype, device):
    return t.reshape(*lead, *tail).to(device=device, dtype=dtype)


class ObjectFactory(abc.ABC):
    """A triangle mesh in its object frame + the closest-point / signed-distance query on it (sdf.py:30-189).

    The reference hands the mesh to open3d's RaycastingScene (Embree, on the CPU, sdf.py:115-118); here the triangle
    soup and the face normals live in HBM and the query is the brute-force `pvamd_mesh_query` kernel.
    """

    def __init__(self, name='', scale=1.0, vis_frame_pos=(0, 0, 0), vis_frame_rot=(0, 0, 0, 1),
                 plausible_suboptimality=0.001, mesh=None, **kwargs):
        """
        :param name: path to the mesh file (.obj / .stl / .npz)
        :param scale: scaling factor for the mesh
        :param vis_frame_pos: position of the mesh in the object frame
        :param vis_frame_rot: xyzw quaternion rotation of the mesh in the object frame
        :param plausible_suboptimality: how much error to tolerate in the SDF
        :param mesh: a mesh_io.TriMesh given directly; scale, vis_frame_pos and vis_frame_rot are then ignored
        """
        self.name = name
        self.scale = scale if scale is not None else 1.0
        self.vis_frame_pos = vis_frame_pos
        self.vis_frame_rot = vis_frame_rot
        self.other_load_kwargs = kwargs
        self.plausible_suboptimality = plausible_suboptimality
        # counter-based stand-in for the reference's unseeded ray jitter (sdf.py:149); change to re-draw
        self.jitter_seed = 0

        self._mesh: typing.Optional[mesh_io.TriMesh] = mesh
        self._face_normals = None
        self._tri_dev = None
        self._normal_dev = None
        self.precompute_sdf()

    def __reduce__(self):
        return partial(self.__class__, scale=self.scale, vis_frame_pos=self.vis_frame_pos,
                       vis_frame_rot=self.vis_frame_rot,
                       plausible_suboptimality=self.plausible_suboptimality, **self.other_load_kwargs), \
            (self.name,)

    @abc.abstractmethod
    def make_collision_obj(self, z, rgba=None):
        """Create collision object of fixed and position along x-y; returns the object ID and bounding box"""

    @abc.abstractmethod
    def get_mesh_resource_filename(self):
        """Return the path to the mesh resource file (.obj, .stl, ...)"""

    def get_mesh_high_poly_resource_filename(self):
        return self.get_mesh_resource_filename()

    def draw_mesh(self, dd, name, pose, rgba, object_id=None):
        """sdf.py:75-78: hand the mesh file and its visual frame to a caller-supplied debug drawer `dd`."""
        frame_pos = np.array(self.vis_frame_pos) * self.scale
        return dd.draw_mesh(name, self.get_mesh_resource_filename(), pose, scale=self.scale, rgba=rgba,
                            object_id=object_id, vis_frame_pos=frame_pos, vis_frame_rot=self.vis_frame_rot)

    def bounding_box(self, padding=0., padding_ratio=0):
        """(3,2) float64 ndarray [[min,max],...] of the vertex AABB, inflated (sdf.py:80-89)."""
        lo, hi = self._mesh.aabb()
        ranges = np.stack((lo, hi), axis=1)
        extents = ranges[:, 1] - ranges[:, 0]
        ranges[:, 0] -= padding + padding_ratio * extents
        ranges[:, 1] += padding + padding_ratio * extents
        return ranges

    def center(self):
        if self._mesh is None:
            self.precompute_sdf()
        return self._mesh.center()

    def precompute_sdf(self):
        """Load + place the mesh (sdf.py:97-113) and derive face normals (sdf.py:119-120), all in float64."""
        if self._mesh is None:
            full_path = os.path.expanduser(self.get_mesh_high_poly_resource_filename())
            if not os.path.exists(full_path):
                raise RuntimeError(f"Expected mesh file does not exist: {full_path}")
            mesh = mesh_io.load_mesh(full_path).scaled(self.scale)
            x, y, z, w = self.vis_frame_rot
            rot = tf.quaternion_to_matrix(torch.tensor([w, x, y, z], dtype=torch.float64)).numpy()
            mesh = mesh.rotated(rot).translated(np.array(self.vis_frame_pos, dtype=np.float64) * np.asarray(self.scale))
            self._mesh = mesh
        if self._face_normals is None:
            self._face_normals = self._mesh.triangle_normals()
            self._tri_dev = None

    # ---- device state ----
    def _mesh_desc(self):
        """Upload + prepare the mesh once per device: triangles in compact patches of 16 / 256 (mesh_io.patch_order: what makes
        the kernels' group and tile spheres tight), per-triangle records, tile spheres, face-id map."""
        dev = _lib.require_gpu()
        if self._tri_dev is None or self._tri_dev.device != dev:
            soup = self._mesh.triangle_soup().astype(np.float32)  # the scene stores float32 vertices
            order = mesh_io.patch_order(soup.mean(axis=1))
            F = soup.shape[0]
            self._tri_dev = torch.from_numpy(np.ascontiguousarray(soup[order])).to(dev)
            face_id = torch.from_numpy(order.astype(np.int32)).to(dev)
            self._normal_dev = torch.from_numpy(np.ascontiguousarray(self._face_normals.astype(np.float32))).to(dev)
            self._rec_dev = torch.empty((max(_lib.rec_floats(F), 4),), dtype=torch.float32, device=dev)
            self._tiles_dev = torch.empty((max(_lib.tiles_floats(F), 4),), dtype=torch.float32,
                                          device=dev)
            self._rec_of_face_dev = torch.empty((max(F, 1),), dtype=torch.int32, device=dev)
            lo, hi = self._mesh.aabb()
            abs_margin = 1e-6 * float(np.abs(self._mesh.vertices).max() + np.linalg.norm(hi - lo)) if F else 0.0
            with _lib.on_device(dev):
                _lib.call("pvamd_mesh_prepare", self._tri_dev, face_id, F, abs_margin, self._rec_dev, self._tiles_dev,
                          self._rec_of_face_dev)
        if getattr(self, "_mesh_desc_cache", None) is not None and self._mesh_desc_cache.rec == self._rec_dev.data_ptr():
            return self._mesh_desc_cache
        desc = _lib.MeshDesc()
        desc.normal = self._normal_dev.data_ptr()
        desc.rec = self._rec_dev.data_ptr()
        desc.tiles = self._tiles_dev.data_ptr()
        desc.rec_of_face = self._rec_of_face_dev.data_ptr()
        desc.F = int(self._tri_dev.shape[0])
        ray = self.bounding_box(padding=1.0)[:, 1]  # sdf.py:147
        for d in range(3):
            desc.ray_dir[d] = float(ray[d])
        self._mesh_desc_cache = desc
        return desc

    def count_exact_pairs(self, enable=True):
        """Measurement hook (pvamd_mesh_t.pair_counters): while enabled, every mesh query / chamfer / cache build over this
        object adds the exact point-triangle tests it executes to a device tensor of two int64 counters (closest-point tests,
        ray tests), which is returned (zeroed).  `enable=False` detaches it.  Results are unaffected."""
        desc = self._mesh_desc()
        if not enable:
            desc.pair_counters = None
            self._pair_counters = None
            return None
        self._pair_counters = torch.zeros((2,), dtype=torch.int64, device=self._rec_dev.device)
        desc.pair_counters = self._pair_counters.data_ptr()
        return self._pair_counters

    def sample_surface(self, n, seed):
        """n area-uniform surface points (float64, on the GPU), the index of the prepared triangle each came from and a
        random key per sample; the draw of sample_mesh_points (sdf.py:643-650)."""
        self._mesh_desc()
        dev = self._tri_dev.device
        if getattr(self, "_area_cdf_dev", None) is None or self._area_cdf_dev.device != dev:
            t = self._tri_dev.double().cpu().numpy()  # areas of the float32 triangles the kernels hold, in their order
            area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
            if not np.isfinite(area).all() or area.sum() <= 0:
                raise ValueError("mesh has no area to sample")
            cdf = np.cumsum(area) / area.sum()
            cdf[-1] = 1.0
            self._area_cdf_dev = torch.from_numpy(cdf).to(dev)
        pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
        face = torch.empty((n,), dtype=torch.int32, device=dev)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.call("pvamd_sample_surface", self._tri_dev, self._area_cdf_dev, int(self._tri_dev.shape[0]), n,
                      ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), pts, face, keys)
        return pts, face, keys

    @property
    def num_faces(self):
        return int(self._mesh.faces.shape[0])

    def _do_object_frame_closest_point(self, points_in_object_frame, compute_normal=False):
        """sdf.py:122-172, the body the reference wraps with handle_batch_input: here the public method takes any batch shape."""
        return self.object_frame_closest_point(points_in_object_frame, compute_normal=compute_normal)

    def object_frame_closest_point(self, points_in_object_frame, compute_normal=False, index_base=0, order=None) -> SDFQuery:
        """
        Closest surface point, signed distance, gradient (and face normal) for points in the object frame
        (sdf.py:122-189).  Any leading batch dimensions; computed in float32 like the reference (sdf.py:132) and
        returned in the caller's dtype on the caller's device (sdf.py:166).

        :param points_in_object_frame: [...] x N x 3 tensor or ndarray
        :param compute_normal: also return the face normal at the closest point
        :param index_base: global index of the first point (keeps the sign jitter identical under sharding)
        :param order: int32 processing order of the flattened points (a permutation that keeps neighbours in space together),
            when the caller already has one; results do not depend on it
        """
        if not torch.is_tensor(points_in_object_frame):
            points_in_object_frame = torch.as_tensor(np.asarray(points_in_object_frame), dtype=torch.float)
        flat, lead, dtype, device = _lib.as_query_points(points_in_object_frame)
        P = flat.shape[0]
        dev = flat.device
        closest = torch.empty((P, 3), dtype=torch.float32, device=dev)
        dist = torch.empty((P,), dtype=torch.float32, device=dev)
        grad = torch.empty((P, 3), dtype=torch.float32, device=dev)
        face = torch.empty((P,), dtype=torch.int32, device=dev)
        normal = torch.empty((P, 3), dtype=torch.float32, device=dev) if compute_normal else None
        desc = self._mesh_desc()
        with _lib.on_device(dev):
            scratch = None
            if P > 0 and getattr(self, "tile_split", True):
                # lets the kernel spread a point group's tiles over several workgroups (every group of a small query, the
                # heavy groups of a large one)
                scratch = _lib.scratch_buffer(_lib.mesh_scratch_bytes(P), dev)
            if order is None and 0 < P <= _lib.mesh_small_points() and scratch is not None:
                # few points: the processing order is worked out inside the query's first launch (one workgroup of it)
                order_scratch = torch.empty((P,), dtype=torch.int32, device=dev)
                _lib.call("pvamd_mesh_query_unordered", desc, flat, P, ctypes.c_uint64(self.jitter_seed), int(index_base),
                          closest, dist, grad, face, normal, order_scratch, scratch)
            else:
                if order is None:
                    order = _lib.morton_order(flat)
                _lib.call("pvamd_mesh_query", desc, flat, order, P, ctypes.c_uint64(self.jitter_seed), int(index_base),
                          closest, dist, grad, face, normal, scratch)
        self._last_face_ids = face
        return SDFQuery(_restore(closest, lead, (3,), dtype, device), _restore(dist, lead, (), dtype, device),
                        _restore(grad, lead, (3,), dtype, device),
                        _restore(normal, lead, (3,), dtype, device) if compute_normal else None)

    def cast_rays(self, origins, directions, t_min=0., t_max=math.inf, world_to_object=None, cull=False) -> MeshRayHits:
        """
        The first triangle every ray o + t d meets, exactly: what cast_rays on the reference's RaycastingScene (sdf.py:115-118)
        answers, for depth, visibility and occlusion checks.  ONE kernel launch (csrc/mesh_ray.hip; include/pvamd.h "Mesh ray
        casting" states the arithmetic), computed in float32 and returned in the promoted dtype of the rays on the origins'
        device; nothing synchronises with the host and nothing carries an autograd graph (inputs that require grad are detached).

        :param origins: [...] x 3, broadcast against `directions`
        :param directions: [...] x 3, of any length: t is the parameter of the caller's direction.  A zero or NaN direction misses
        :param t_min: hits with a smaller t are passed over
        :param t_max: hits with a larger t are passed over
        :param world_to_object: None (the rays are in the object frame), (4, 4) or (B, 4, 4) matrices that take the rays' frame to
            the object frame.  A batch prepends B to every output shape: the rays are shared by the poses.  Normals come back in
            the rays' frame, which is meaningful for rigid poses only
        :param cull: False: every ray is tested against every triangle.  True: the culled contract (include/pvamd.h "Mesh ray
            casting, culled"): a triangle counts only if the ray also passes a float32 test against the bounding spheres of the
            triangle's tile and group of the prepared mesh and the hit's point lies in them, and whole tiles and groups are skipped -- the same bits on rays in
            general position at a fraction of the cost, and next to none of the plain mode's rounding-noise hits for rays that
            lie in a triangle's plane; on such rays the result may depend on how the mesh was sorted
        :return: MeshRayHits(t, face_ids, normals, uv); t = inf and face_ids = -1 where nothing is hit
        """
        if not isinstance(cull, bool):
            raise TypeError(f"cull must be a bool, got {type(cull).__name__}")
        t_min, t_max = _ray_window(t_min, t_max)
        o, d, lead, dtype = _ray_inputs(origins, directions)
        device = o.device
        poses, batch = None, ()
        if world_to_object is not None:
            poses = world_to_object.get_matrix() if hasattr(world_to_object, "get_matrix") else world_to_object
            poses = poses if torch.is_tensor(poses) else torch.as_tensor(poses)
            if poses.dim() not in (2, 3) or tuple(poses.shape[-2:]) != (4, 4):
                raise ValueError(f"world_to_object must be (4, 4) or (B, 4, 4), got {tuple(poses.shape)}")
            batch = tuple(poses.shape[:-2])
        desc = self._mesh_desc()
        dev = self._rec_dev.device
        o = o.reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        d = d.reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        R = o.shape[0]
        B = 1
        if poses is not None:
            poses = poses.detach().reshape(-1, 4, 4).to(device=dev, dtype=torch.float32).contiguous()
            B = poses.shape[0]
        t = torch.empty((B, R), dtype=torch.float32, device=dev)
        face = torch.empty((B, R), dtype=torch.int32, device=dev)
        normal = torch.empty((B, R, 3), dtype=torch.float32, device=dev)
        uv = torch.empty((B, R, 2), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.call("pvamd_mesh_ray_cast_culled" if cull else "pvamd_mesh_ray_cast", desc, o, d, R, poses, B, t_min, t_max, t, face,
                      normal, uv)
        shape = batch + lead
        return MeshRayHits(_restore(t, shape, (), dtype, device), face.reshape(shape).to(device=device, dtype=torch.int64),
                           _restore(normal, shape, (3,), dtype, device), _restore(uv, shape, (2,), dtype, device))

    def render_depth(self, intrinsics, height, width, camera_pose, max_depth=math.inf, cull=False):
        """
        Depth images of the mesh from pinhole cameras: the image TSDFVolume.integrate and OccupancyMap take.

        :param intrinsics: (fx, fy, cx, cy) or a 3 x 3 matrix; pixel (row, col) is centred on (u, v) = (col, row)
        :param camera_pose: (4, 4) or (K, 4, 4): the camera's pose in the object frame; it looks along +z, x right, y down
        :param max_depth: hits deeper than this count as no return
        :param cull: cast_rays' `cull`: True renders under the culled contract
        :return: (K,) H x W float32 on the GPU: z-depth along the optical axis, t * (direction in the camera frame)_z of
            camera_rays' unit directions, and exactly 0 -- integrate's "no return" -- where nothing was hit
        """
        from pytorch_volumetric_amd import tsdf
        if not isinstance(cull, bool):
            raise TypeError(f"cull must be a bool, got {type(cull).__name__}")
        if isinstance(max_depth, bool) or not isinstance(max_depth, numbers.Real):
            raise TypeError(f"max_depth must be a Python real number, got {type(max_depth).__name__}")
        if not max_depth > 0:
            raise ValueError(f"max_depth must be positive, got {max_depth!r}")
        pose = camera_pose if torch.is_tensor(camera_pose) else torch.as_tensor(camera_pose)
        if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) != (4, 4):
            raise ValueError(f"camera_pose must be (4, 4) or (K, 4, 4), got {tuple(pose.shape)}")
        tsdf._check_intrinsics(intrinsics)  # before a GPU is asked for
        dev = _lib.require_gpu()
        origins, directions, local = tsdf._pinhole(intrinsics, height, width, pose.detach().to(device=dev, dtype=torch.float32))
        hits = self.cast_rays(origins, directions, cull=cull)
        depth = hits.t * local[..., 2]
        return torch.where((hits.face_ids >= 0) & (depth <= float(max_depth)), depth, torch.zeros_like(depth))


class MeshObjectFactory(ObjectFactory):
    """sdf.py:192-214"""

    def __init__(self, mesh_name='', path_prefix='', **kwargs):
        self.path_prefix = path_prefix
        # strip the package:// prefix when a path prefix is given (loading URDF-referenced meshes manually)
        self.strip_package_prefix = path_prefix != ''
        super(MeshObjectFactory, self).__init__(mesh_name, **kwargs)

    def __reduce__(self):
        return partial(self.__class__, path_prefix=self.path_prefix, scale=self.scale, vis_frame_pos=self.vis_frame_pos,
                       vis_frame_rot=self.vis_frame_rot,
                       plausible_suboptimality=self.plausible_suboptimality, **self.other_load_kwargs), \
            (self.name,)

    def make_collision_obj(self, z, rgba=None):
        return None, None

    def get_mesh_resource_filename(self):
        mesh_path = self.name
        if self.strip_package_prefix:
            mesh_path = mesh_path.replace("package://", "")
        return os.path.join(self.path_prefix, mesh_path)


class ObjectFrameSDF(abc.ABC):
    """The drop-in protocol (sdf.py:217-246)."""

    @abc.abstractmethod
    def __call__(self, points_in_object_frame):
        """
        :param points_in_object_frame: [...] x N x 3 points in the object frame
        :return: ([...] x N signed distance, [...] x N x 3 gradient pointing towards higher SDF values)
        """

    @abc.abstractmethod
    def surface_bounding_box(self, padding=0., padding_ratio=0.):
        """(min,max) per dimension of the 0-level set, inflated by padding + padding_ratio*extent."""

    def outside_surface(self, points_in_object_frame, surface_level=0):
        sdf_values, _ = self.__call__(points_in_object_frame)
        return sdf_values > surface_level

    def ray_cast(self, origins, directions, t_min=0., t_max=math.inf, hit_tolerance=1e-3, step_scale=1., max_steps=128,
                 differentiable=False):
        """Sphere tracing: where each ray origins + t * directions first meets the surface (include/pvamd.h "Ray casting").

        :param origins, directions: (..., 3), broadcast against each other and promoted to one dtype (the dtype and device rules
            of __call__; an integer dtype counts as float32).  Directions are meant to be unit length: any other length scales
            the step.
        :param t_min, t_max: the march starts at t_min and stops as MISS once the next t would pass t_max (+inf allowed)
        :param hit_tolerance: a ray stops as HIT at the first evaluated point whose value is <= hit_tolerance
        :param step_scale: each step advances t by step_scale * value
        :param max_steps: at most this many evaluations per ray (1 .. 65535); a ray still marching then reports MAX_STEPS
        :return: RayCast(t, status, values, gradients, steps) of shapes (...), (...), (...), (..., 3), (...): t is the parameter of
            the last evaluated point (t_min when none was), values / gradients are the bits __call__ returns there (NaN when none
            was), status is uint8 (RAY_MISS, RAY_HIT, RAY_MAX_STEPS, RAY_INVALID: the query returned NaN), steps int32.  Each real
            scalar is rounded once to the rays' dtype, and every product and sum is rounded separately in it.  No rays give empty
            results.
        :param differentiable: must be a bool.  False (the default), grad mode off or nothing that requires grad: the result
            carries no autograd graph, and rays that require grad are accepted and detached.  True with origins or directions
            that require grad: t -- and only t -- gains a grad_fn, every output keeping the bits of the non-differentiable call.
            The gradient is the surface-normal linearisation at the hit point (include/pvamd.h "Ray casting: gradient of the hit
            distance"), not autograd through the loop: with n = gradients and c = n . d, a ray with status RAY_HIT and c < 0
            gives dt/do = -n / c and dt/dd = -t n / c, every other ray exactly zero.  A grazing hit (c -> 0-) gives a large
            gradient by construction; weighting it is the caller's job.  Double backward is not supported.

        This is the loop in torch around __call__ -- every SDF has it; it is not a hot path and synchronises once per step.
        CachedSDF and ComposedSDF run it as one HIP kernel where they can (csrc/ray_cast.hip)."""
        args = _ray_args(t_min, t_max, hit_tolerance, step_scale, max_steps)
        o, d, lead, dtype = _ray_inputs(origins, directions)
        return self._ray_cast_generic(o, d, lead, dtype, args, _ray_graph(differentiable, origins, directions, lead))

    def _ray_cast_generic(self, o, d, lead, dtype, args, graph=None):
        """ray_cast after the argument checks: the torch loop around __call__ on the rays' own device.  graph (_ray_graph): t
        leaves with the contract's gradient w.r.t. the rays attached, its bits unchanged."""
        dev = o.device if o.device.type != "cpu" else d.device
        o = o.reshape(-1, 3).to(device=dev, dtype=dtype)
        d = d.reshape(-1, 3).to(device=dev, dtype=dtype)
        with torch.no_grad():
            t, status, v, g, steps = _ray_march(self.__call__, o, d, *args)
        if graph is not None:
            from pytorch_volumetric_amd import autograd
            t = autograd.RayHitDistance.apply(graph[0], graph[1], d, t, status, g)
        return RayCast(t.reshape(lead), status.reshape(lead), v.reshape(lead), g.reshape(*lead, 3), steps.reshape(lead))

    def get_voxel_view(self, voxels=None, dtype=torch.float, device='cpu'):
        """The SDF sampled at the centres of a voxel grid, addressed by coordinates (sdf.py:248-264): ONE batched
        query over every centre.  Default grid: 0.01 m over surface_bounding_box(padding=0.1).  Points outside the
        grid's range are answered by the SDF itself (`invalid_value=self.__call__`)."""
        from pytorch_volumetric_amd.voxel_containers import ValueRangeView, VoxelGrid
        if voxels is None:
            voxels = VoxelGrid(0.01, self.surface_bounding_box(padding=0.1).cpu().numpy(), dtype=dtype, device=device)
        pts = voxels.get_voxel_center_points()
        sdf_val, _ = self.__call__(pts.unsqueeze(0))
        sampled = sdf_val.reshape([len(coord) for coord in voxels.coords])
        return ValueRangeView(sampled, voxels.range_per_dim, invalid_value=lambda q: self.__call__(q)[0])

    def get_filtered_points(self, unary_filter, voxels=None, dtype=torch.float, device='cpu'):
        """N x 3 voxel centres whose SDF value passes `unary_filter` (sdf.py:266-282), e.g. `lambda v: v <= 0` for
        the interior."""
        view = self.get_voxel_view(voxels, dtype=dtype, device=device)
        indices = unary_filter(view.raw_data).nonzero().reshape(-1)
        # raw_data is flat: back to one index per dimension (C order), then to coordinates
        key = torch.stack(torch.unravel_index(indices, view.shape), dim=-1)
        return view.ensure_value_key(key)


class SphereSDF(ObjectFrameSDF):
    """Closed-form sphere at the origin (sdf.py:285-299); a handful of stock elementwise ops, kept in torch."""

    def __init__(self, radius):
        self.radius = radius

    def __call__(self, points_in_object_frame):
        dist_to_origin = torch.linalg.norm(points_in_object_frame, dim=-1)
        return dist_to_origin - self.radius, points_in_object_frame / (dist_to_origin.unsqueeze(-1) + 1e-12)

    def surface_bounding_box(self, padding=0., padding_ratio=0.):
        length = self.radius + padding + padding_ratio * self.radius
        return torch.tensor([[-length, length], [-length, length], [-length, length]])


class MeshSDF(ObjectFrameSDF):
    """SDF straight from the mesh (sdf.py:302-329): one brute-force point x triangle kernel launch per call."""

    def __init__(self, obj_factory: ObjectFactory, vis=None):
        self.obj_factory = obj_factory
        self.vis = vis  # accepted for signature compatibility; debug drawing is out of scope

    def surface_bounding_box(self, **kwargs):
        return torch.tensor(self.obj_factory.bounding_box(**kwargs))

    def __call__(self, points_in_object_frame):
        res = self.obj_factory.object_frame_closest_point(points_in_object_frame)
        return res.distance, res.gradient


class OutOfBoundsStrategy(enum.Enum):
    """sdf.py:436-438"""
    LOOKUP_GT_SDF = 0
    BOUNDING_BOX = 1


class VoxelView:
    """What CachedSDF.voxels exposes of the reference's TorchMultidimView: raw_data, shape and the three index
    methods used at sdf.py:537-540, all evaluated by the `pvamd_voxel_index` kernel."""

    def __init__(self, owner: "CachedSDF"):
        self._owner = owner
        self.shape = owner._view.shape[:owner._dim]

    @property
    def raw_data(self):
        if self._owner._dim == 2:  # the planar cache is stored as two identical z layers: expose one
            nx, ny, _ = self._owner._view.shape
            return self._owner._packed.reshape(nx, ny, 2, 4)[:, :, 0, 0].reshape(-1)
        return self._owner._packed[:, 0]

    def _index(self, points, want_key=False, want_flat=False, want_valid=False):
        flat, lead, _, device = _lib.as_query_points(self._owner._lift(points), self._owner._packed.device, keep_f64=True)
        P = flat.shape[0]
        key = torch.empty((P, 3), dtype=torch.int64, device=flat.device) if want_key else None
        ravel = torch.empty((P,), dtype=torch.int64, device=flat.device) if want_flat else None
        valid = torch.empty((P,), dtype=torch.uint8, device=flat.device) if want_valid else None
        desc = self._owner._grid_desc()
        with _lib.on_device(flat.device):
            _lib.call("pvamd_voxel_index", desc, flat, P, key, ravel, valid, f64=flat.dtype == torch.float64)
        d = self._owner._dim
        return (key.reshape(*lead, 3)[..., :d] if want_key else None, ravel.reshape(*lead) if want_flat else None,
                valid.reshape(*lead).bool() if want_valid else None)

    def ensure_index_key(self, points):
        return self._index(points, want_key=True)[0]

    def ravel_multi_index(self, key, shape=None):
        shape = shape or self.shape
        if len(shape) == 2:
            return key[..., 0] * shape[1] + key[..., 1]
        return (key[..., 0] * shape[1] + key[..., 1]) * shape[2] + key[..., 2]

    def get_valid_values(self, points):
        return self._index(points, want_valid=True)[2]


INTERPOLATIONS = ("nearest", "trilinear")


def _check_interpolation(value, dim):
    if value not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {INTERPOLATIONS}, got {value!r}")
    if value == "trilinear" and dim != 3:
        raise ValueError(f'interpolation="trilinear" needs a 3-D cache, this one is {dim}-dimensional (bilinear planar caches '
                         "are not supported)")


def _require_nearest(sdf, what):
    """Entry points with nearest-voxel kernels only: a trilinear cache (or a composition over one) raises rather than being
    answered with nearest-voxel bits."""
    leaves = getattr(sdf, "sdfs", None)
    for s in (leaves if leaves is not None else [sdf]):
        mode = getattr(s, "interpolation", "nearest")
        if mode != "nearest":
            raise ValueError(f'{what} supports interpolation="nearest" only; this {"composition has a leaf" if leaves is not None else "cache"} '
                             f'with interpolation="{mode}" (use __call__)')


class CachedSDF(ObjectFrameSDF):
    """SDF by nearest-voxel lookup in a precomputed (value, gradient) grid (sdf.py:441-614).

    HBM layout: one 16-byte (val, gx, gy, gz) record per voxel, C order; a query is one gather plus the fused
    out-of-bounds branch (`pvamd_cached_query`)."""

    def __init__(self, object_name, resolution, range_per_dim, gt_sdf: ObjectFrameSDF,
                 out_of_bounds_strategy=OutOfBoundsStrategy.BOUNDING_BOX,
                 device="cpu", clean_cache=False,
                 debug_check_sdf=False, cache_path="sdf_cache.pkl", interpolation="nearest"):
        """
        :param object_name: readable name; combined with resolution and range into the cache key
        :param resolution: side length of each voxel
        :param range_per_dim: (min, max) per dimension
        :param gt_sdf: SDF used to fill the cache and (LOOKUP_GT_SDF) to answer out-of-range queries
        :param out_of_bounds_strategy: LOOKUP_GT_SDF or BOUNDING_BOX (distance to the surface bounding box)
        :param device: device the results are returned on (the lookup itself always runs on the MI355X)
        :param clean_cache: ignore an existing cache entry and recompute
        :param debug_check_sdf: verify the cache against gt_sdf after building / on every query
        :param cache_path: torch.save'd dict {name: (val[nx,ny,nz], grad[n,3])}, same format as the reference
        :param interpolation: "nearest" (the reference's nearest-voxel lookup, the default) or "trilinear" (opt-in, 3-D caches
            only: continuous value and gradient in range, differentiable w.r.t. the points; see README "Interpolated queries").
            A query-time choice: the cache and its key do not depend on it.
        """
        _check_interpolation(interpolation, len(range_per_dim))
        self.interpolation = interpolation
        self.device = device
        self.out_of_bounds_strategy = out_of_bounds_strategy
        self.gt_sdf = gt_sdf
        self.resolution = resolution
        self.debug_check_sdf = debug_check_sdf

        bb = np.array(range_per_dim)
        num_voxel = (bb[:, 1] - bb[:, 0]) // resolution
        if min(num_voxel) < 10:
            logger.warning(f"Resolution {resolution} is too high for {object_name}, only getting {num_voxel} voxels.")

        range_per_dim = get_divisible_range_by_resolution(resolution, range_per_dim)
        self.ranges = range_per_dim
        self.name = f"{object_name} {resolution} {tuple(range_per_dim)}"

        val, grad, built = None, None, None
        data = {}
        if cache_path is not None and os.path.exists(cache_path):
            data = torch.load(cache_path, weights_only=False) or {}
            try:
                val, grad = data[self.name]
                logger.info("cached sdf for %s loaded from %s", self.name, cache_path)
            except (ValueError, KeyError):
                logger.info("cached sdf invalid %s from %s, recreating", self.name, cache_path)

        if val is None or clean_cache:
            if gt_sdf is None:
                raise RuntimeError("Cached SDF did not find the cache and requires an initialize queryable SDF")
            # per-axis coordinates exactly as the reference builds them (fp32 arange on the host); their cartesian
            # product is formed on the GPU so that a 10^7-voxel grid never exists in host memory
            coords, _ = get_coordinates_and_points_in_grid(self.resolution, self.ranges, get_points=False)
            dev_q = _lib.require_gpu()
            built = self._build_from_mesh(gt_sdf, coords, dev_q)
            if built is None:
                built = self._copy_from_occupancy(gt_sdf, self.resolution, self.ranges, coords, dev_q)
            if built is not None:
                # a plain MeshSDF: centres, processing order, mesh kernel and packing in <= 3 launches (pvamd_cache_build); an
                # OccupancySDF over this very lattice: its records;
                # `val` / `grad` are views of the packed records -- what the reference stores and pickles
                val, grad = built[:, 0].reshape([len(coord) for coord in coords]), built[:, 1:4]
            else:
                pts = torch.cartesian_prod(*[c.to(dev_q) for c in coords])
                sdf_val, sdf_grad = gt_sdf(pts)  # any other ground truth: asked at every voxel centre
                val = sdf_val.reshape([len(coord) for coord in coords])
                grad = sdf_grad.reshape(-1, len(coords))  # (N, d): what the reference stores and pickles (sdf.py:505, squeeze(0))
            if cache_path is not None:
                data[self.name] = val.contiguous().cpu(), grad.contiguous().cpu()  # (views of the packed records after a fused build)
                torch.save(data, cache_path)
                logger.info("caching sdf for %s to %s", self.name, cache_path)

        # The kernels are three-dimensional.  A planar (d = 2) cache -- the protocol allows it, sdf.py:222 -- is stored as
        # two identical z layers over z in [-1, 1] and queried at z = 0: x / y index arithmetic, range test and the
        # bounding-box branch (t_z = 0) are the planar statements, the z component of every output is dropped.
        self._dim = len(self.ranges)
        if self._dim not in (2, 3):
            raise ValueError(f"CachedSDF works in 2 or 3 dimensions, got a {self._dim}-dimensional range")
        view_ranges = list(self.ranges)
        if self._dim == 2:
            one = type(self.ranges[0][0])(1.0) if isinstance(self.ranges[0][0], (float, np.floating)) else 1.0
            view_ranges = view_ranges + [(-one, one)]
            val = torch.stack((val, val), dim=-1)
            g2 = grad.reshape(-1, 2)
            g3 = torch.cat((g2, torch.zeros_like(g2[:, :1])), dim=1)
            grad = torch.stack((g3, g3), dim=1).reshape(-1, 3)
        self._view = RangeView(view_ranges, val.shape)
        dev = _lib.require_gpu()
        if built is not None and self._dim == 3 and built.device == dev:
            self._packed = built  # the mesh kernel wrote the records themselves
        else:
            val_d = val.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            grad_d = grad.to(device=dev, dtype=torch.float32).contiguous().reshape(-1, 3)
            self._packed = torch.empty((val_d.shape[0], 4), dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                _lib.call("pvamd_pack_grid", val_d, grad_d, val_d.shape[0], self._packed)
        self.voxels = VoxelView(self)
        self.voxels_grad = self._packed[:, 1:]
        self.bb = self.surface_bounding_box().to(device=dev)
        if self._dim == 2 and self.bb.shape[0] == 2:
            self.bb = torch.cat((self.bb, torch.tensor([[-1.0, 1.0]], dtype=self.bb.dtype, device=dev)), dim=0)

        if self.debug_check_sdf and gt_sdf is not None:
            _, pts = get_coordinates_and_points_in_grid(self.resolution, self.ranges)
            q, _ = self(pts)
            ok = self.voxels.get_valid_values(pts).to(q.device)  # fp32 boundary centres can round outside a f64 range
            centre_val = val[..., 0] if self._dim == 2 else val
            assert torch.allclose(centre_val.reshape(-1).to(q.device, q.dtype)[ok], q[ok])  # voxel centres map to themselves

    @staticmethod
    def _build_from_mesh(gt_sdf, coords, dev):
        """The cache of a plain MeshSDF in at most three launches (pvamd_cache_build; sdf.py:498-516 on the device): packed
        (n, 4) records on `dev`, or None when the ground truth is anything else (a subclass, a planar grid, a mesh elsewhere)."""
        if type(gt_sdf) is not MeshSDF or len(coords) != 3 or not isinstance(gt_sdf.obj_factory, ObjectFactory):
            return None
        obj = gt_sdf.obj_factory
        shape = [len(c) for c in coords]
        n = shape[0] * shape[1] * shape[2]
        if n == 0 or n > 2 ** 31 - 1:
            return None
        with _lib.on_device(dev):
            desc = obj._mesh_desc()
            if obj._rec_dev.device != dev:
                return None
            # one host -> device copy for the three coordinate arrays (fp32, exactly as voxel.py:20-25 builds them)
            allc = torch.cat([c.to(torch.float32) for c in coords]).to(dev)
            cx, cy, cz = allc[:shape[0]], allc[shape[0]:shape[0] + shape[1]], allc[shape[0] + shape[1]:]
            packed = torch.empty((n, 4), dtype=torch.float32, device=dev)
            pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
            order = torch.empty((n,), dtype=torch.int32, device=dev)
            scratch = _lib.scratch_buffer(_lib.mesh_scratch_bytes(n), dev) \
                if getattr(obj, "tile_split", True) else None
            _lib.call("pvamd_cache_build", desc, cx, cy, cz, shape[0], shape[1], shape[2], ctypes.c_uint64(obj.jitter_seed),
                      packed, pts, order, scratch)
        return packed

    @staticmethod
    def _copy_from_occupancy(gt_sdf, resolution, ranges, coords, dev):
        """The cache of an OccupancySDF whose lattice is the cache's own: a copy of the field's packed (n, 4) records as they are,
        on `dev`.  None for any other ground truth or lattice (the field is then asked at every voxel centre)."""
        from pytorch_volumetric_amd.occupancy import OccupancySDF
        if not isinstance(gt_sdf, OccupancySDF) or not gt_sdf.same_lattice(resolution, ranges, [len(c) for c in coords]):
            return None
        return gt_sdf._records.to(device=dev, copy=True)

    _PLAN_ATTRS = frozenset(("device", "out_of_bounds_strategy", "debug_check_sdf", "_packed", "bb", "interpolation"))

    def __setattr__(self, name, value):
        if name == "interpolation":
            _check_interpolation(value, self.__dict__.get("_dim", 3))
        if name in CachedSDF._PLAN_ATTRS:
            _lib.EPOCH[0] += 1  # call plans (this object's and those of compositions over it) are rebuilt on next use
            if name in ("bb", "_packed"):
                # ... and so are the descriptors that hold the box / the cache pointer by value: this object's, and (through
                # the generation number in ComposedSDF._leaf_grids' key) the device arrays of compositions over it
                self.__dict__.pop("_desc_by_mode", None)
                self.__dict__["_desc_gen"] = self.__dict__.get("_desc_gen", 0) + 1
        object.__setattr__(self, name, value)

    def surface_bounding_box(self, **kwargs):
        return self.gt_sdf.surface_bounding_box(**kwargs)

    def _fast_plan(self):
        """What the fast path of __call__ needs, resolved once per configuration epoch: float32 points that already sit
        contiguous on the grid's GPU, the fused BOUNDING_BOX strategy, results wanted on that same GPU -> one C-ABI call
        between two allocations.  None when this object cannot take it."""
        dev = self._packed.device
        ok = self._dim == 3 and self.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX and \
            not self.debug_check_sdf and self.interpolation == "nearest" and _lib.same_gpu(self.device, dev)
        plan = None
        if ok:
            desc = self._grid_desc()
            fast = _lib.fastcall()
            plan = (dev, dev.index, ctypes.byref(desc), _lib.load().pvamd_cached_query, desc, fast,
                    _lib.entry_address("pvamd_cached_query") if fast is not None else 0, ctypes.addressof(desc))
        object.__setattr__(self, "_plan", (_lib.EPOCH[0], plan))
        return plan

    def _lift(self, points):
        """planar caches: (..., 2) query points -> (..., 3) with z = 0 (see __init__)"""
        if getattr(self, "_dim", 3) == 3:
            return points
        if not torch.is_tensor(points):
            points = torch.as_tensor(points)
        if points.shape[-1] != 2:
            raise ValueError(f"this cache is planar: query points must have last dimension 2, got {tuple(points.shape)}")
        return torch.cat((points, torch.zeros_like(points[..., :1])), dim=-1)

    def _grid_desc(self, oob_mode=None):
        """pvamd_grid_t for this cache (built once per out-of-bounds mode: filling it costs ~40 host scalar reads)."""
        mode_key = self.out_of_bounds_strategy if oob_mode is None else oob_mode
        cache = self.__dict__.setdefault("_desc_by_mode", {})
        hit = cache.get(mode_key)
        if hit is not None and hit.vox == self._packed.data_ptr():
            return hit
        desc = _lib.GridDesc()
        desc.vox = self._packed.data_ptr()
        self._view.fill(desc)
        bb = self.bb.to(dtype=torch.float32, device="cpu")
        bb64 = self.bb.to(dtype=torch.float64, device="cpu")  # float64 queries: sdf.py:556-557 casts bb to the query dtype
        for d in range(3):
            desc.bb_min[d], desc.bb_max[d] = bb[d, 0].item(), bb[d, 1].item()
            desc.dbb_min[d], desc.dbb_max[d] = bb64[d, 0].item(), bb64[d, 1].item()
        mode = self.out_of_bounds_strategy if oob_mode is None else oob_mode
        desc.oob_mode = _lib.OOB_BOUNDING_BOX if mode == OutOfBoundsStrategy.BOUNDING_BOX else _lib.OOB_LOOKUP_GT_SDF
        _lib.call("pvamd_grid_finalize", desc)
        cache[mode_key] = desc
        return desc

    def __call__(self, points_in_object_frame):
        """sdf.py:535-591"""
        p = points_in_object_frame
        # gradients (autograd.py): only when grad mode is on and the points require grad -- one attribute read otherwise
        if getattr(p, "requires_grad", False) and torch.is_grad_enabled() and self._dim == 3 and \
                self.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX:
            from pytorch_volumetric_amd import autograd
            return autograd.cached_query(self, p)
        # the common call of a planner's inner loop -- float32 points already contiguous on the grid's GPU -- skips every
        # conversion below: two allocations in the final shapes and one C-ABI call (~7.5 us instead of ~18 us of host time per
        # call, 5.1 us through query_into; the kernel itself takes 5.2 us for a million points, 2.4 us for 15,251)
        cached = self.__dict__.get("_plan")
        plan = cached[1] if cached is not None and cached[0] == _lib.EPOCH[0] else self._fast_plan()
        if plan is not None and plan[5] is not None and type(p) is torch.Tensor:
            # csrc/fastcall.cpp: the same checks, allocations and C-ABI call as the branch below, in C++ (None: not its case)
            out = plan[5].cached_call(plan[6], plan[7], plan[1], p)
            if out is not None:
                return out
        if plan is not None and type(p) is torch.Tensor and p.dtype is torch.float32 and p.device == plan[0] and \
                p.is_contiguous() and p.dim() >= 1 and p.shape[-1] == 3 and _lib.current_device_index() == plan[1]:
            # (p is float32, contiguous, on plan[0]: empty_like / new_empty give the same tensors as torch.empty(shape, dtype=,
            # device=) without the keyword parsing -- 1.3 + 1.8 us instead of 3.6 + 3.8 on this container's CPU)
            val = p.new_empty((p.shape[0],)) if p.dim() == 2 else p.new_empty(p.shape[:-1])
            grad = torch.empty_like(p)
            rc = plan[3](plan[2], p.data_ptr(), val.numel(), val.data_ptr(), grad.data_ptr(), None,
                         _lib.current_raw_stream(plan[1]))
            if rc != 0:
                _lib.check(rc, "pvamd_cached_query")
            return val, grad
        # the launch happens on the GPU that holds the grid, whatever device is current in the calling code
        # float64 points are looked up in float64 (index arithmetic, range test and bounding-box branch all promote to
        # the query dtype in the reference: sdf.py:537-540,545-547,556-571); everything else is computed in float32
        flat, lead, dtype, _ = _lib.as_query_points(self._lift(points_in_object_frame), self._packed.device, keep_f64=True)
        dev = flat.device
        lookup_gt = self.out_of_bounds_strategy == OutOfBoundsStrategy.LOOKUP_GT_SDF
        val, grad, oob = self._forward(flat, want_oob=lookup_gt)
        if lookup_gt:
            idx = oob.nonzero().squeeze(-1)  # sdf.py:552-554: ground truth on the out-of-range subset only
            if idx.numel() > 0:
                v_gt, g_gt = self.gt_sdf(flat[idx][:, :self._dim])
                val[idx] = v_gt.to(device=dev, dtype=flat.dtype)
                grad[idx, :self._dim] = g_gt.to(device=dev, dtype=flat.dtype)
        val = _restore(val, lead, (), dtype, self.device)
        grad = _restore(grad[:, :self._dim], lead, (self._dim,), dtype, self.device)
        if self.debug_check_sdf:
            val_gt = self.gt_sdf(points_in_object_frame)[0].to(device=val.device, dtype=val.dtype)
            within = self.voxels.get_valid_values(points_in_object_frame).to(val.device)
            assert torch.all((torch.abs(val - val_gt) < self.resolution)[within])
        return val, grad

    def query_into(self, points, out_val, out_grad):
        """Allocation-free form of __call__ for inner loops and graph capture: `points` fp32 contiguous (P,3) on the
        GPU, results written into the caller's fp32 (P,) / (P,3) buffers.  BOUNDING_BOX strategy only.  One C-ABI call,
        one kernel launch on the current stream."""
        # the same resolved plan as __call__'s fast path: when every argument already is what the kernel takes, the checks below
        # (which raise the descriptive errors) and their context manager are skipped -- an eager call costs the host ~6 us
        # instead of ~10 (the kernel: 2.4-5.2 us)
        cached = self.__dict__.get("_plan")
        plan = cached[1] if cached is not None and cached[0] == _lib.EPOCH[0] else self._fast_plan()
        if plan is not None and type(points) is torch.Tensor and type(out_val) is torch.Tensor and type(out_grad) is torch.Tensor:
            if plan[5] is not None and plan[5].cached_into(plan[6], plan[7], plan[1], points, out_val, out_grad):
                return  # csrc/fastcall.cpp: the checks below and the call, in C++
            dev, f32 = plan[0], torch.float32
            if points.dtype is f32 and out_val.dtype is f32 and out_grad.dtype is f32 and points.device == dev and \
                    out_val.device == dev and out_grad.device == dev and points.dim() == 2 and points.is_contiguous() and \
                    out_val.is_contiguous() and out_grad.is_contiguous() and _lib.current_device_index() == plan[1]:
                P = points.shape[0]
                if points.shape[1] == 3 and out_val.shape == (P,) and out_grad.shape == (P, 3):
                    rc = plan[3](plan[2], points.data_ptr(), P, out_val.data_ptr(), out_grad.data_ptr(), None,
                                 _lib.current_raw_stream(plan[1]))
                    if rc != 0:
                        _lib.check(rc, "pvamd_cached_query")
                    return
        _require_nearest(self, "query_into")
        if self.out_of_bounds_strategy != OutOfBoundsStrategy.BOUNDING_BOX:
            raise ValueError("query_into needs the fused BOUNDING_BOX strategy")
        if not (points.is_cuda and points.dtype == torch.float32 and points.is_contiguous()):
            raise ValueError("query_into needs contiguous fp32 points on the GPU")
        if not (points.device == self._packed.device == out_val.device == out_grad.device):
            raise _lib.PvamdError(f"query_into: the grid lives on {self._packed.device}; points / outputs are on "
                                  f"{points.device} / {out_val.device} / {out_grad.device}")
        P = points.shape[0]
        if out_val.shape != (P,) or out_grad.shape != (P, 3) or out_val.dtype != torch.float32 or \
                out_grad.dtype != torch.float32 or not (out_val.is_contiguous() and out_grad.is_contiguous()):
            raise ValueError("query_into needs contiguous fp32 outputs of shape (P,) and (P,3)")
        desc = self._grid_desc()  # cached per mode and cache pointer, dropped by __setattr__ when `bb` / the cache change
        with _lib.on_device(points.device):
            _lib.call("pvamd_cached_query", desc, points, P, out_val, out_grad, None)

    def _forward(self, flat, want_oob):
        """(val, grad, oob) of contiguous (P, 3) points on the grid's GPU (float64 stays float64) by this cache's interpolation:
        one launch; oob (uint8, 1 = out of range) only with want_oob, None otherwise."""
        P = flat.shape[0]
        val = torch.empty((P,), dtype=flat.dtype, device=flat.device)
        grad = torch.empty((P, 3), dtype=flat.dtype, device=flat.device)
        oob = torch.empty((P,), dtype=torch.uint8, device=flat.device) if want_oob else None
        desc = self._grid_desc()
        with _lib.on_device(flat.device):
            _lib.call("pvamd_cached_query" if self.interpolation == "nearest" else "pvamd_cached_query_interp",
                      desc, flat, P, val, grad, oob, f64=flat.dtype == torch.float64)
        return val, grad, oob

    def ray_cast(self, origins, directions, t_min=0., t_max=math.inf, hit_tolerance=1e-3, step_scale=1., max_steps=128,
                 differentiable=False):
        """ObjectFrameSDF.ray_cast (arguments, results and contract there; include/pvamd.h "Ray casting") against this cache, in the
        cache's interpolation.  A 3-D BOUNDING_BOX cache with float32 or float64 rays is ONE kernel launch (csrc/ray_cast.hip:
        a lane per ray, the whole march in registers, nothing but the results written) with nothing that synchronises with the
        host, so it can be captured in a graph; LOOKUP_GT_SDF caches and other dtypes run the torch loop around __call__.
        Planar caches raise.  Results are returned on this cache's device; they carry no autograd graph unless differentiable=True
        and a ray input requires grad: then t carries the gradient of the hit distance, and on the one-kernel path its backward
        is one elementwise kernel (csrc/ray_cast_backward.hip) from the forward's own t, status and gradients.

        A nearest cache is piecewise constant -- one voxel-centre sample per voxel -- so the march can overshoot the surface
        by up to half a voxel diagonal: interpolation="trilinear" or step_scale < 1 is the remedy."""
        args = _ray_args(t_min, t_max, hit_tolerance, step_scale, max_steps)
        o, d, lead, dtype = _ray_inputs(origins, directions)
        graph = _ray_graph(differentiable, origins, directions, lead)
        if self._dim != 3:
            raise ValueError("ray_cast needs a 3-D cache, this one is planar")
        if self.out_of_bounds_strategy != OutOfBoundsStrategy.BOUNDING_BOX or self.debug_check_sdf or \
                dtype not in (torch.float32, torch.float64):
            return self._ray_cast_generic(o, d, lead, dtype, args, graph)
        if graph is not None:
            from pytorch_volumetric_amd import autograd
            return autograd.ray_cast(self, graph, o, d, lead, dtype, args)
        return self._ray_cast_fused(o, d, lead, dtype, args)[0]

    def _ray_cast_fused(self, o, d, lead, dtype, args):
        """One pvamd_cached_ray_cast[_f64] call.  Returns the RayCast, then what the backward needs: the flat rays the kernel read
        and its five output buffers."""
        dev = self._packed.device
        o = o.reshape(-1, 3).to(device=dev, dtype=dtype).contiguous()
        d = d.reshape(-1, 3).to(device=dev, dtype=dtype).contiguous()
        R = o.shape[0]
        out = _ray_outputs((R,), dtype, dev)
        with _lib.on_device(dev):
            _lib.call("pvamd_cached_ray_cast", self._grid_desc(), _lib.LEAF_MODES[self.interpolation], o, d, R, *args, *out,
                      f64=dtype == torch.float64)
        return _ray_result(out, lead, self.device), {"o": o, "d": d, "out": out}

    def extract_mesh(self, level=0.0, normals=True):
        """The surface `value == level` of the cache as a Surface (vertices, faces, normals on the GPU), by naive surface nets over
        the cache's own records and lattice (surface.extract_surface): whatever filled the cache -- a mesh, an occupancy or TSDF
        field -- and whatever the interpolation mode and out-of-bounds strategy.  normals=True interpolates unit normals from the
        cached gradients.  `.to_trimesh()` of the result is what MeshObjectFactory(mesh=...) and mesh_io.save_obj take."""
        from pytorch_volumetric_amd import surface
        level, normals = surface.check_level(level), surface.check_normals(normals)
        if self._dim != 3:
            raise ValueError("extract_mesh needs a 3-D cache, this one is planar")
        surface.check_shape(self._view.shape, "the cache")
        return surface.surface_of_records(self._grid_desc(), self._packed, None, level, normals)

    def outside_surface(self, points_in_object_frame, surface_level=0):
        """sdf.py:593-602 (trilinear caches: the interpolated value > surface_level in range, True out of range)"""
        flat, lead, _, _ = _lib.as_query_points(self._lift(points_in_object_frame), self._packed.device, keep_f64=True)
        if self.interpolation == "trilinear":
            val, _, oob = self._forward(flat, want_oob=True)
            return ((oob != 0) | (val > surface_level)).reshape(*lead).to(device=self.device)
        out = torch.empty((flat.shape[0],), dtype=torch.uint8, device=flat.device)
        desc = self._grid_desc()
        with _lib.on_device(flat.device):
            _lib.call("pvamd_cached_outside", desc, flat, flat.shape[0], float(surface_level), out, f64=flat.dtype == torch.float64)
        return out.reshape(*lead).bool().to(device=self.device)

    def _fallback_sdf_value_func(self, *args, **kwargs):
        """sdf.py:530-533: the ground-truth value on this SDF's device (what a view answers outside its grid)"""
        sdf_val, _ = self.gt_sdf(*args, **kwargs)
        return sdf_val.to(device=self.device)

    def get_voxel_view(self, voxels=None, dtype=torch.float, device='cpu'):
        """sdf.py:604-614: the cache's own view, or the ground-truth SDF sampled over another voxel grid (points outside that
        grid are answered by the ground-truth SDF: _fallback_sdf_value_func, sdf.py:530-533)."""
        if voxels is None:
            return self.voxels
        if self.gt_sdf is None:
            raise RuntimeError("Cannot sample another voxel grid without a ground truth SDF")
        from pytorch_volumetric_amd.voxel_containers import ValueRangeView
        pts = voxels.get_voxel_center_points()
        sdf_val, _ = self.gt_sdf(pts.unsqueeze(0))
        sampled = sdf_val.to(device=self.device).reshape([len(coord) for coord in voxels.coords])
        return ValueRangeView(sampled, voxels.range_per_dim,
                              invalid_value=self._fallback_sdf_value_func)


class PreparedPoints:
    """A query point set sorted once along the Hilbert curve (ComposedSDF.prepare_points).
    points: (P, 3) float32, caller order, on the leaves' GPU.  order: int32 (P,), order[j] = caller index of sorted position j.
    inverse: int32 (P,), inverse[i] = sorted position of caller point i.  sorted_points = points[order]."""

    def __init__(self, points, order, inverse, sorted_points, padded_points, lead, dtype):
        self.points, self.order, self.inverse = points, order, inverse
        self.sorted_points, self.padded_points = sorted_points, padded_points
        self.lead, self.dtype = lead, dtype

    def __len__(self):
        return int(self.points.shape[0])


# ComposedSDF's choices between its query paths (module globals: the eager fast path of __call__ reads them on every call).
# The INLINE_EXACT tuning hint (ComposedSDF._leaf_grids): leaf grids that together fit the 4 MB L2 of an XCD make the kernel
# instruction-bound, larger ones gather-bound.
_XCD_L2_BYTES = 4 << 20
_INLINE_EXACT = _lib.COMPOSED_INLINE_EXACT
_TILE_POINTS = _lib.TILE_POINTS
# Regrouping under group_points "auto" (ComposedSDF._grouping_pays): wherever the library itself would launch its wave-tile
# kernel were regrouping off -- asked of the library (remembered per shape), not restated here.
_composed_kernel, _NO_GROUPING, _WAVE_TILE = _lib.composed_query_kernel, _lib.COMPOSED_NO_GROUPING, _lib.CO_KERNEL_WAVE_TILE
# The spatial sort under bucket_points "auto" (ComposedSDF._bucketing_pays has the measurements): gather-bound grids, enough
# configurations to share one sort, enough points, the (A, P) 16-byte records of the sorted pass within 8 GiB -- and the
# leaf-grid bytes one configuration's query can touch (_footprint_bytes) above 8 MB: a planar slice stays below and is not sorted.
_SORT_MIN_CONFIGS = 8
_SORT_MIN_POINTS = 32768
_SORT_MAX_RECORD_BYTES = 8 << 30
_SORT_MIN_FOOTPRINT_BYTES = 8 << 20


class ComposedSDF(ObjectFrameSDF):
    """Minimum over S rigidly placed leaf SDFs (sdf.py:332-433).

    When every leaf is a BOUNDING_BOX CachedSDF (the RobotSDF / README configuration) the whole call -- transform
    into each leaf frame, lookup, rotate the gradient back, first-minimum over leaves -- is ONE fused kernel
    (`pvamd_composed_query`) that never materialises the reference's (S, A, P, 3) intermediates."""

    def __init__(self, sdfs: typing.Sequence[ObjectFrameSDF], obj_frame_to_each_frame):
        """
        :param sdfs: S object-frame SDFs
        :param obj_frame_to_each_frame: [B*]S transforms (Transform3d / object with get_matrix() / (.,4,4) tensor)
            from the shared object frame to each leaf frame, leaf-major when batched
        """
        self.sdfs = sdfs
        self._tf_obj, self._tf_matrix = None, None  # obj_frame_to_link_frame: the Transform3d (built when asked for) / its matrices
        self.link_frame_to_obj_frame = None
        self.tsf_batch = None
        self._tf_dev = None
        self._grids_dev = None
        self._grids_key = None
        self._plan = None
        self.set_transforms(obj_frame_to_each_frame)

    @property
    def obj_frame_to_link_frame(self):
        """The [B*]S object -> leaf transforms as a Transform3d (sdf.py:343,377).  A planner that re-configures every step
        hands over a bare (S*A, 4, 4) stack; the object around it is built when somebody asks (1.2 us per step otherwise)."""
        if self._tf_obj is None and self._tf_matrix is not None:
            # a stack its owner re-writes in place is handed out as a copy: what the caller holds keeps its configuration
            volatile = self.__dict__.get("_tf_volatile", False)
            self._tf_obj = tf.Transform3d(matrix=self._tf_matrix.clone() if volatile else self._tf_matrix)
        return self._tf_obj

    @obj_frame_to_link_frame.setter
    def obj_frame_to_link_frame(self, value):
        self._tf_obj = value
        self._tf_matrix = None if value is None else tf.as_matrix(value)
        self._tf_grad = self._tf_matrix is not None and self._tf_matrix.requires_grad

    def ith_transform_slice(self, i):
        if self.tsf_batch is None:
            return slice(i, i + 1)
        total_to_slice = math.prod(list(self.tsf_batch))
        return slice(i * total_to_slice, (i + 1) * total_to_slice)

    def set_transforms(self, tsf, batch_dim=None, known_rigid=False):
        """sdf.py:370-383.  An un-given batch is inferred as (S_tsf // S,) -- the reference computes a float there
        (sdf.py:379) and cannot slice with it; only its explicit batch_dim path works."""
        if tsf is None:
            self.obj_frame_to_link_frame, self.link_frame_to_obj_frame = None, []
            self.tsf_batch, self._tf_dev, self._tf_dev64, self._rigid = batch_dim, None, None, True
            self._tf_grad = False
            return
        m = tf.as_matrix(tsf)
        S, S_tsf = len(self.sdfs), m.shape[0]
        if batch_dim is None:
            if S_tsf % S != 0:
                raise ValueError(f"{S_tsf} transforms cannot be split over {S} SDFs")
            batch_dim = None if S_tsf == S else (S_tsf // S,)
        else:
            batch_dim = tuple(int(b) for b in batch_dim)
            if math.prod(batch_dim) * S != S_tsf:
                raise ValueError(f"{S_tsf} transforms != {S} SDFs x batch {batch_dim}")
        # validated: now commit
        self._tf_volatile = False
        self.tsf_batch, self._tf_dev, self._tf_dev64 = batch_dim, None, None
        self._tf_obj, self._tf_matrix = (tsf if hasattr(tsf, "get_matrix") else None), m
        # a differentiable stack (RobotSDF under a q that requires grad, poses being optimised): __call__ routes through
        # autograd.ComposedQuery; the kernels always read its detached storage (_tf_device)
        self._tf_grad = m.requires_grad
        # The reference inverts with a general matrix inverse (sdf.py:380).  Rigid stacks (every RobotSDF stack, and
        # what the fused kernel's leaf-culling spheres and R^T gradient rotation assume) use the exact R^T form;
        # anything else -- scale, shear, a drifted rotation -- takes the general inverse and the unfused path, whose
        # x = L p + t and g_obj = L^T g_leaf are valid for any affine transform.
        # (known_rigid: RobotSDF's stack is rigid by construction -- FK composed with R^T inverses -- and re-checking it
        # costs three device->host synchronisations per set_joint_configuration: 0.19 -> 0.46 ms for 200 configurations)
        self._rigid = True if known_rigid else tf.is_rigid(m)
        # the inverse frames only serve surface_bounding_box: built when first asked for (a planner that sets a new joint
        # configuration every step paid 0.09 of 0.16 ms of host time for them)
        self._inverse_of, self._inverse_frames = m, None

    def invalidate_transforms(self):
        """The transform stack handed to set_transforms was re-written IN PLACE (RobotSDF.configure_and_query_into): drop every
        copy derived from its old contents -- the float64 widening of the float64 query path, the inverse frames of
        surface_bounding_box, the Transform3d wrapper.  The float32 device stack aliases the caller's tensor and stays."""
        self._tf_dev64 = None
        self._inverse_frames = None
        self._tf_volatile = True
        if self._tf_matrix is not None:
            self._inverse_of = self._tf_matrix
        self._tf_obj = None
        if self._tf_dev is not None and self._tf_matrix is not None and self._tf_dev.data_ptr() != self._tf_matrix.data_ptr():
            self._tf_dev = None  # (a converted copy, not an alias: rebuilt on the next query)

    @property
    def link_frame_to_obj_frame(self):
        """sdf.py:380-383: the S inverse transforms, leaf by leaf."""
        if self._inverse_frames is None and self._inverse_of is not None:
            m = self._inverse_of
            inv = tf.rigid_inverse(m) if self._rigid else torch.linalg.inv(m)
            self._inverse_frames = [tf.Transform3d(matrix=inv[self.ith_transform_slice(i)]) for i in range(len(self.sdfs))]
        return self._inverse_frames

    @link_frame_to_obj_frame.setter
    def link_frame_to_obj_frame(self, frames):
        self._inverse_of, self._inverse_frames = None, frames

    def surface_bounding_box(self, **kwargs):
        """sdf.py:347-368, including its choice of transforming only the min-row and the max-row of each leaf box."""
        bounds = []
        for i, sdf in enumerate(self.sdfs):
            t = self.link_frame_to_obj_frame[i]
            pts = sdf.surface_bounding_box(**kwargs)
            pts = t.transform_points(pts.to(dtype=t.dtype, device=t.device).transpose(0, 1))
            if self.tsf_batch is not None and len(pts.shape) == 2:
                pts = pts.unsqueeze(0)
            bounds.append(pts)
        bounds = torch.stack(bounds)
        if self.tsf_batch is not None:
            dims = (0,) + tuple(range(2, len(bounds.shape) - 1))
        else:
            dims = tuple(range(len(bounds.shape) - 1))
        return torch.stack((bounds.amin(dim=dims), bounds.amax(dim=dims)), dim=-1)

    # ---- fused path ----
    def _fused_mode(self):
        """The leaf mode of the fused kernels ("nearest" / "trilinear") when every leaf is a 3-D BOUNDING_BOX CachedSDF with that
        interpolation and the transforms are rigid; None otherwise (compositions that mix the modes take the generic path)."""
        if not self.sdfs or not getattr(self, "_rigid", True):
            return None
        modes = {s.interpolation if isinstance(s, CachedSDF) and s._dim == 3 and
                 s.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX else None for s in self.sdfs}
        return modes.pop() if len(modes) == 1 else None

    def _fusable(self):
        """The nearest fused kernels serve this composition (what the nearest-only entry points and dist.ShardedSDF ask)."""
        return self._fused_mode() == "nearest"

    bucket_points = "auto"  # True / False / "auto": sort the query points spatially before the fused kernel (see __call__)
    group_points = "auto"   # True / False / "auto": regroup the points spatially inside chunks (pvamd_composed_query_grouped)

    def _direct_flags(self):
        """flags of a pvamd_composed_query call: the grid-size hint, plus "no regrouping" when group_points is False (the entry point
        regroups inside its workgroups on its own where that pays: composed_query_fused)"""
        return self._query_flags | (_lib.COMPOSED_NO_GROUPING if self.group_points is False else 0)

    def _grouping_pays(self, A, P, flags):
        """The chunk-grouped kernel (round 6): one small sort launch shared by the A configurations, then waves of
        neighbouring points -- most leaf visits become all-outside instead of paying the look-up half for a few lanes (C4:
        0.68 -> 0.5 ms).  "auto": the regime of the wave-tile kernel (several configurations, enough tiles to fill the
        chip: what pvamd_composed_query_kernel answers under NO_GROUPING) on L2-resident grids; a single configuration cannot
        amortise the extra pass over the points."""
        gp = self.group_points
        if gp is False or flags != 0 or P < _lib.group_chunk_points():
            return False
        if gp is True:
            return True
        return _composed_kernel(A, P, _NO_GROUPING) == _WAVE_TILE

    def _bucketing_pays(self, A, P, points=None):
        """Sorting the points costs a sort + a second pass over the outputs (~0.6 ms for 200 x 262,144); it pays when
        the leaf grids are far larger than L2, so that gather locality decides the time, and the sort is shared by enough
        configurations.  Measured on the README-size robot (8 x 21 MB grids, A = 200, P = 262,144 random points):
        4.9 ms direct, 1.7 ms bucketed; with 100 KB grids the kernel is instruction-bound and bucketing only adds its
        overhead (0.82 -> 1.1 ms).  With `points`, "auto" also looks at what the query can touch at all: a planar slice
        (512 x 512 points in grid order: 0.87 ms direct, 1.25 ms bucketed) cuts each leaf grid in a plane whose cells stay
        in L2 whatever the order, so it is not sorted; a 64^3 grid in grid order (2.3 ms direct, 1.5 ms bucketed) fills
        the volume and is (tools/coherent_probe.py, profiles/r03_probes.txt)."""
        if self.bucket_points != "auto":
            return bool(self.bucket_points) and P >= _TILE_POINTS
        if not self._fusable():
            return False
        self._leaf_grids(self._owner_device())  # derives _query_flags from the grid sizes
        # (the fast path of __call__ carries this line too, on the same names: a call through a shared method cost it 0.1 us)
        if not (self._query_flags & _INLINE_EXACT and A >= _SORT_MIN_CONFIGS and P >= _SORT_MIN_POINTS and
                A * P * 16 <= _SORT_MAX_RECORD_BYTES):
            return False
        return points is None or self._footprint_bytes(points) > _SORT_MIN_FOOTPRINT_BYTES

    def _footprint_bytes(self, flat):
        """Upper estimate of the leaf-grid bytes one configuration's query touches: the cells of the finest leaf grid that
        the points' bounding box covers (at least one cell thick per axis, at most one per point), a 64-byte line each,
        for every leaf.  One small kernel + one device->host read (~25 us) per call: not remembered -- a planner that allocates
        a fresh point tensor every step gets the same address back from the caching allocator, so no cheap key tells a new
        query from the last one."""
        box = torch.empty((2, 3), dtype=torch.float32, device=flat.device)
        _lib.call("pvamd_points_aabb", flat, flat.shape[0], box)
        lo, hi = box.cpu().double().unbind(0)
        extent = (hi - lo).clamp_min(0.0)
        res = min(float(s._view.dres.min()) for s in self.sdfs)
        cells = 1.0
        for d in range(3):
            e = float(extent[d])
            cells *= max(1.0, e / res) if math.isfinite(e) else float("inf")
        return min(cells, float(flat.shape[0])) * 64.0 * len(self.sdfs)

    def _owner_device(self):
        """The one GPU every leaf grid lives on (the fused kernel reads all of them through raw pointers)."""
        devs = {s._packed.device for s in self.sdfs}
        if len(devs) != 1:
            raise _lib.PvamdError(f"ComposedSDF: leaf grids live on different devices {sorted(map(str, devs))}")
        return next(iter(devs))

    def _leaf_grids(self, dev):
        key = tuple((id(s), s._packed.data_ptr(), s.__dict__.get("_desc_gen", 0)) for s in self.sdfs) + (str(dev),)
        if self._grids_dev is None or self._grids_key != key:
            host = [s._grid_desc() for s in self.sdfs]
            descs = (_lib.GridDesc * len(self.sdfs))(*host)
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
            self._grids_dev = raw.to(dev)
            self._grids_key = key
            # tuning hint (never changes a result, include/pvamd.h).  Grids that fit the 4 MB L2 of an XCD make the kernel
            # instruction-bound: keep the exact-division fallback out of its hot loop (flagged points are redone after
            # it).  Larger grids make it gather-bound and, with their larger coordinate / resolution ratios, flag far more
            # visits (21 MB README-size link grids: 22 % of the wave passes): the inline fallback is cheaper there.
            grid_bytes = sum(int(s._packed.numel()) * 4 for s in {id(s): s for s in self.sdfs}.values())
            self._query_flags = _lib.COMPOSED_INLINE_EXACT if grid_bytes > _XCD_L2_BYTES else 0
        return self._grids_dev

    def _tf_device(self, dev):
        if self._tf_dev is None or self._tf_dev.device != dev:
            self._tf_dev = self._tf_matrix.detach().to(device=dev, dtype=torch.float32).contiguous()
        return self._tf_dev

    def _call_plan(self):
        """What the fast path of __call__ needs about the LEAVES (not the transforms: a planner sets those before every
        query), resolved once per (configuration epoch, leaf list): every leaf a BOUNDING_BOX CachedSDF on one GPU, the
        descriptor array there, results wanted on that GPU.  None when the composition cannot take the fast path."""
        sdfs = self.sdfs
        key = (_lib.EPOCH[0], *map(id, sdfs))
        cached = self._plan
        if cached is not None and cached[0] == key:
            return cached[1]
        plan = None
        if len(sdfs) > 0 and all(isinstance(s, CachedSDF) and s._dim == 3 and
                                 s.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX and
                                 s.interpolation == "nearest" for s in sdfs):
            devs = {s._packed.device for s in sdfs}
            if len(devs) == 1:
                dev = next(iter(devs))
                with _lib.on_device(dev):
                    grids = self._leaf_grids(dev)
                if _lib.same_gpu(sdfs[0].device, dev):
                    fast = _lib.fastcall()
                    plan = (dev, dev.index, grids.data_ptr(), len(sdfs), _lib.load().pvamd_composed_query, grids, fast,
                            _lib.entry_address("pvamd_composed_query") if fast is not None else 0)
        self._plan = (key, plan)
        return plan

    def __call__(self, points_in_object_frame):
        """sdf.py:392-433.  Returns (A..., B..., N) / (A..., B..., N, 3) with a transform batch, and -- like the
        reference -- FLAT (P,) / (P, 3) without one."""
        p = points_in_object_frame
        # gradients (autograd.py): a flag stored by set_transforms and one attribute read of the points in front of the fast paths
        if (self._tf_grad or getattr(p, "requires_grad", False)) and torch.is_grad_enabled():
            mode = self._fused_mode()
            if mode is not None:
                from pytorch_volumetric_amd import autograd
                return autograd.composed_query(self, p, mode)
        plan = self._call_plan()
        # float32 points already contiguous on the leaves' GPU, fused leaves, rigid transforms, no sort wanted: two
        # allocations in the final shapes around one C-ABI call (RobotSDF.__call__ in a planner's loop)
        if plan is not None and type(p) is torch.Tensor and p.dtype is torch.float32 and p.device == plan[0] and \
                p.is_contiguous() and p.dim() >= 1 and p.shape[-1] == 3 and self._rigid and \
                self._tf_matrix is not None and _lib.current_device_index() == plan[1]:
            P = p.numel() // 3
            batch = self.tsf_batch
            A = math.prod(batch) if batch is not None else 1
            bp = self.bucket_points
            flags = self._query_flags
            # the arithmetic half of _bucketing_pays, inline (its footprint probe waits in the general path)
            sort = (flags & _INLINE_EXACT and A >= _SORT_MIN_CONFIGS and P >= _SORT_MIN_POINTS and
                    A * P * 16 <= _SORT_MAX_RECORD_BYTES) if bp == "auto" else (bool(bp) and P >= _TILE_POINTS)
            if P > 0 and not sort:
                dev = plan[0]
                tfd = self._tf_dev
                if tfd is None or tfd.device != dev:
                    tfd = self._tf_device(dev)
                grouping = self._grouping_pays(A, P, flags)
                if plan[6] is not None and not grouping and (batch is None or len(batch) > 0):  # csrc/fastcall.cpp: the allocations and the call below, in C++
                    out = plan[6].composed_call(plan[7], plan[2], plan[3], tfd.data_ptr(), A, batch if batch is not None else (),
                                                flags | (_lib.COMPOSED_NO_GROUPING if self.group_points is False else 0), plan[1], p)
                    if out is not None:
                        return out
                # (p is float32 on dev: new_empty = torch.empty(shape, dtype=, device=) without the keyword parsing)
                if batch is not None:
                    val = p.new_empty((*batch, *p.shape[:-1]))
                    grad = p.new_empty((*batch, *p.shape))
                else:
                    val = p.new_empty((P,))
                    grad = p.new_empty((P, 3))
                if grouping:
                    scratch = _lib.group_points(p.view(-1, 3))
                    _lib.check(_lib.load().pvamd_composed_query_grouped(plan[2], plan[3], tfd.data_ptr(), A, scratch.data_ptr(), P,
                                                                        val.data_ptr(), grad.data_ptr(), None, flags,
                                                                        _lib.current_raw_stream(plan[1])),
                               "pvamd_composed_query_grouped")
                    return val, grad
                rc = plan[4](plan[2], plan[3], tfd.data_ptr(), A, p.data_ptr(), P, val.data_ptr(), grad.data_ptr(), None,
                             flags | (_lib.COMPOSED_NO_GROUPING if self.group_points is False else 0),
                             _lib.current_raw_stream(plan[1]))
                if rc != 0:
                    _lib.check(rc, "pvamd_composed_query")
                return val, grad
        mode = self._fused_mode()
        if not torch.is_tensor(points_in_object_frame):
            points_in_object_frame = torch.as_tensor(points_in_object_frame)
        if mode == "trilinear" or (mode == "nearest" and points_in_object_frame.dtype == torch.float64):
            val, grad, _, _, _ = self._fused_forward(points_in_object_frame, mode)
            return val, grad
        S = len(self.sdfs)
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        pts_shape = points_in_object_frame.shape
        out_device = points_in_object_frame.device
        fused = mode == "nearest"
        if not fused and points_in_object_frame.dtype == torch.float64:
            return self._generic_f64(points_in_object_frame, S, A)
        flat, _, dtype, _ = _lib.as_query_points(points_in_object_frame, self._owner_device() if fused else None)
        P = flat.shape[0]
        dev = flat.device
        if fused:
            out_device = self.sdfs[0].device  # leaves return on their own device (sdf.py:546)
            val = torch.empty((A, P), dtype=torch.float32, device=dev)
            grad = torch.empty((A, P, 3), dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                grids = self._leaf_grids(dev)
                if self._bucketing_pays(A, P, flat):
                    # one spatial sort (Hilbert curve) of the shared point set, amortised over the A configurations; the kernel then
                    # sees spatially compact wave tiles and a second pass restores the caller's point order
                    _, inv, spts = _lib.morton_order(flat, min_points=0, want_inverse=True, want_sorted=True)
                    Pp = _lib.whole_tiles(P)
                    if Pp != P:  # whole tiles: pad with copies of the last point (never read back)
                        spts = torch.cat((spts, spts[-1:].expand(Pp - P, 3))).contiguous()
                    scratch = torch.empty((A, Pp, 4), dtype=torch.float32, device=dev)
                    _lib.call("pvamd_composed_query_bucketed", grids, S, self._tf_device(dev), A, spts, inv, P, Pp, scratch,
                              val, grad, self._query_flags)
                elif self._grouping_pays(A, P, self._query_flags):
                    scratch = _lib.group_points(flat)
                    _lib.call("pvamd_composed_query_grouped", grids, S, self._tf_device(dev), A, scratch, P, val, grad, None,
                              self._query_flags)
                else:
                    _lib.call("pvamd_composed_query", grids, S, self._tf_device(dev), A, flat, P, val, grad, None,
                              self._direct_flags())
        else:
            val, grad = self._generic(flat, S, A)
        if self.tsf_batch is not None:
            val = val.reshape(*self.tsf_batch, *pts_shape[:-1])
            grad = grad.reshape(*self.tsf_batch, *pts_shape[:-1], 3)
        else:
            val, grad = val.reshape(-1), grad.reshape(-1, 3)
        return val.to(device=out_device, dtype=dtype), grad.to(device=out_device, dtype=dtype)

    def _fused_forward(self, points, mode, want_leaf=False, configs=None):
        """One launch of the fused kernel of leaf mode `mode` over all the points, without sorting or regrouping them: float64
        points with the float64 widening of the stack (sdf.py:395-431 over sdf.py:545-547; the reference's own bmm would refuse
        the mixed dtypes), anything else in float32.  Returns (val, grad) in the caller's shapes on the leaves' device, the (A, P)
        leaf ids (want_leaf), the flat points and the stack the kernel read (what the backward needs).  `configs` (a device index
        tensor into the flattened batch): those configurations only, (count, P) / (count, P, 3) left on the leaves' GPU."""
        S = len(self.sdfs)
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        dev = self._owner_device()
        f64 = points.dtype == torch.float64
        flat, tfd, dtype = self._fused_inputs(points, dev)
        if configs is not None:
            tfd, A = tfd.reshape(S, A, 4, 4)[:, configs].contiguous(), configs.numel()
        P = flat.shape[0]
        val = torch.empty((A, P), dtype=flat.dtype, device=dev)
        grad = torch.empty((A, P, 3), dtype=flat.dtype, device=dev)
        leaf = torch.empty((A, P), dtype=torch.int32, device=dev) if want_leaf else None
        if P > 0:
            with _lib.on_device(dev):
                grids = self._leaf_grids(dev)
                flags = (self._direct_flags(),) if mode == "nearest" and not f64 else ()  # pvamd_composed_query alone takes them
                _lib.call("pvamd_composed_query" if mode == "nearest" else "pvamd_composed_query_interp",
                          grids, S, tfd, A, flat, P, val, grad, leaf, *flags, f64=f64)
        if configs is not None:
            return val, grad, leaf, flat, tfd
        if self.tsf_batch is not None:
            val = val.reshape(*self.tsf_batch, *points.shape[:-1])
            grad = grad.reshape(*self.tsf_batch, *points.shape[:-1], 3)
        else:
            val, grad = val.reshape(-1), grad.reshape(-1, 3)
        out_device = self.sdfs[0].device  # leaves return on their own device (sdf.py:546)
        return val.to(device=out_device, dtype=dtype), grad.to(device=out_device, dtype=dtype), leaf, flat, tfd

    def _fused_inputs(self, points, dev):
        """(flat points, transform stack, result dtype) as the fused kernels read them: float64 points with the float64 widening
        of the stack, anything else in float32."""
        if points.dtype == torch.float64:
            flat = points.detach().reshape(-1, 3).to(device=dev, dtype=torch.float64).contiguous()
            tfd = self.__dict__.get("_tf_dev64")
            if tfd is None or tfd.device != dev:
                tfd = self._tf_dev64 = self._tf_matrix.detach().to(device=dev, dtype=torch.float64).contiguous()
            return flat, tfd, torch.float64
        flat, _, dtype, _ = _lib.as_query_points(points, dev)
        return flat, self._tf_device(dev), dtype

    # ---- minimum over points ----
    def min_over_points(self, points, per_leaf=False):
        """For every configuration, the point of `points` where the composition comes closest, without the (A, P) field.

        :param points: (..., 3); the leading dimensions are flattened into P, and `indices` index that flattened order
        :param per_leaf: False: the minimum of the composed value (what __call__ returns); True: one minimum per leaf s
            (leaf s = self.sdfs[s], alone under its own transforms)
        :return: MinOverPoints(values, indices, gradients) of shapes B, B, B + (3,) (per_leaf: B + (S,), B + (S,), B + (S, 3)),
            B the transform batch shape (() without one).  indices are int64; values / gradients have the dtype __call__
            returns.  Ties go to the smallest index, a NaN counts as the minimum, -0.0 and +0.0 tie; values / gradients are the
            bits __call__ (per_leaf: the one-leaf composition) gives at that index.  Differentiable w.r.t. the points and the
            transforms (a RobotSDF's joint values) when grad mode is on and they require grad; indices carry no gradient.

        Fused compositions (_fused_mode(): every leaf a BOUNDING_BOX CachedSDF of one interpolation, rigid transforms) with float32
        or float64 points run two HIP kernels (csrc/min_over_points.hip) whose extra memory is O(A S + A P / 4096); anything else
        is __call__ plus a torch reduction under the same contract."""
        if not isinstance(per_leaf, bool):
            raise TypeError(f"per_leaf must be True or False, got {per_leaf!r}")
        if not torch.is_tensor(points):
            points = torch.as_tensor(points)
        if points.dim() < 1 or points.shape[-1] != 3:
            raise ValueError(f"query points must have last dimension 3, got {tuple(points.shape)}")
        if points.numel() == 0:
            raise ValueError("min_over_points: no points (the minimum over an empty set is undefined, as for torch.min)")
        if self._tf_matrix is None:
            raise ValueError("min_over_points needs the transforms to be set")
        mode = self._fused_mode()
        if mode is None or points.dtype not in (torch.float32, torch.float64):
            return self._min_over_points_generic(points, per_leaf)
        if (self._tf_grad or points.requires_grad) and torch.is_grad_enabled():
            from pytorch_volumetric_amd import autograd
            return autograd.min_over_points(self, points, mode, per_leaf)
        val, idx, grad = self._min_over_points_fused(points, mode, per_leaf)[:3]
        return MinOverPoints(val, idx, grad)

    def _min_over_points_fused(self, points, mode, per_leaf):
        """One pvamd_composed_min_over_points[_f64] call.  Returns (values, indices, gradients) in the result shapes on the leaves'
        device, then what the backward needs: the (A, Z) indices and leaf ids, the flat points and the stack the kernels read."""
        S = len(self.sdfs)
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        A = math.prod(batch)
        dev = self._owner_device()
        flat, tfd, dtype = self._fused_inputs(points, dev)
        P, Z = flat.shape[0], S if per_leaf else 1
        val = torch.empty((A, Z), dtype=flat.dtype, device=dev)
        grad = torch.empty((A, Z, 3), dtype=flat.dtype, device=dev)
        idx = torch.empty((A, Z), dtype=torch.int64, device=dev)
        leaf = torch.empty((A, Z), dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            scratch = _lib.scratch_buffer(_lib.min_over_points_scratch_bytes(S, A, P, per_leaf), dev)
            _lib.call("pvamd_composed_min_over_points", grids, S, tfd, A, flat, P, _lib.LEAF_MODES[mode], per_leaf,
                      val, grad, idx, leaf, scratch, f64=flat.dtype == torch.float64)
        shape = batch + ((S,) if per_leaf else ())
        out_device = self.sdfs[0].device  # leaves return on their own device (sdf.py:546)
        return (val.reshape(shape).to(device=out_device, dtype=dtype), idx.reshape(shape).to(device=out_device),
                grad.reshape(*shape, 3).to(device=out_device, dtype=dtype), idx, leaf, flat, tfd)

    def _min_over_points_generic(self, points, per_leaf):
        """Compositions the kernels do not serve (other leaves, mixed modes, other dtypes): __call__ (per leaf: the one-leaf
        composition) and a torch reduction under the same contract -- not a hot path.  Differentiable through __call__."""
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        if per_leaf:
            parts = []
            for s in range(len(self.sdfs)):
                one = ComposedSDF([self.sdfs[s]], None)
                one.set_transforms(self._tf_matrix[self.ith_transform_slice(s)], batch_dim=self.tsf_batch,
                                   known_rigid=self._rigid)
                parts.append(one._min_over_points_generic(points, False))
            return MinOverPoints(*(torch.stack(t, dim=len(batch)) for t in zip(*parts)))
        A = math.prod(batch)
        val, grad = self(points)
        val, grad = val.reshape(A, -1), grad.reshape(A, -1, 3)
        idx = first_argmin(val.detach())
        v = val.gather(1, idx.unsqueeze(1)).squeeze(1)
        g = grad.gather(1, idx.view(A, 1, 1).expand(A, 1, 3)).squeeze(1)
        return MinOverPoints(v.reshape(batch), idx.reshape(batch), g.reshape(*batch, 3))

    # ---- ray casting ----
    def ray_cast(self, origins, directions, t_min=0., t_max=math.inf, hit_tolerance=1e-3, step_scale=1., max_steps=128,
                 differentiable=False):
        """ObjectFrameSDF.ray_cast (arguments and contract there; include/pvamd.h "Ray casting") against the composition under every
        configuration: the rays are given in the composition's object frame and shared by all configurations.

        :return: RayCast(t, status, values, gradients, steps) of shapes B + (...) (gradients B + (..., 3)), B the transform batch
            shape (() without one) and (...) the broadcast shape of origins and directions without its last dimension.  Row a is,
            bit for bit, the loop over configuration a alone, with the values and gradients __call__ returns.  Without
            differentiable=True the result carries no autograd graph: rays (and transforms) that require grad are accepted and
            detached.
        :param differentiable: True, with grad mode on and origins, directions or the transforms (a RobotSDF's joint values)
            requiring grad: t gains a grad_fn, with the same bits (ObjectFrameSDF.ray_cast; include/pvamd.h "Ray casting: gradient
            of the hit distance").  The rays' gradients sum over the configurations; the winning leaf s's transform M gets
            dM[:3, :3] = w gamma x^T and dM[:3, 3] = w gamma per contributing pair (gamma = M[:3, :3] n, w = -upstream / c), summed
            over the rays.  Fused compositions run one HIP backward (csrc/ray_cast_backward.hip: fixed-order float64 sums, bitwise
            reproducible, at most 64 leaves).  Any other composition differentiates w.r.t. the rays only and raises ValueError
            when its transforms require grad.

        Fused compositions (_fused_mode(): every leaf a BOUNDING_BOX CachedSDF of one interpolation, rigid transforms) with float32
        or float64 rays run ONE kernel (csrc/ray_cast.hip: a lane per configuration and ray) that writes nothing but the results
        and does not synchronise with the host, so the call can be captured in a graph; anything else runs the torch loop around
        __call__, one configuration at a time.  Nearest leaves can overshoot the surface by up to half a voxel diagonal (see
        CachedSDF.ray_cast)."""
        args = _ray_args(t_min, t_max, hit_tolerance, step_scale, max_steps)
        o, d, lead, dtype = _ray_inputs(origins, directions)
        if self._tf_matrix is None:
            raise ValueError("ray_cast needs the transforms to be set")
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        graph = _ray_graph(differentiable, origins, directions, lead, self._tf_grad)
        mode = self._fused_mode()
        if mode is None or dtype not in (torch.float32, torch.float64):
            return self._ray_cast_per_configuration(o, d, lead, dtype, args, batch, graph)
        if graph is not None:
            from pytorch_volumetric_amd import autograd
            return autograd.ray_cast(self, graph, o, d, lead, dtype, args)
        return self._ray_cast_fused(o, d, lead, dtype, args)[0]

    def _ray_cast_fused(self, o, d, lead, dtype, args):
        """One pvamd_composed_ray_cast[_f64] call.  Returns the RayCast, then what the backward needs: the flat rays and the stack
        the kernel read, the leaf descriptors and the five output buffers."""
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        mode = self._fused_mode()
        S, A = len(self.sdfs), math.prod(batch)
        dev = self._owner_device()
        o = o.reshape(-1, 3).to(device=dev, dtype=dtype).contiguous()
        d = d.reshape(-1, 3).to(device=dev, dtype=dtype).contiguous()
        _, tfd, _ = self._fused_inputs(o, dev)
        R = o.shape[0]
        out = _ray_outputs((A, R), dtype, dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            _lib.call("pvamd_composed_ray_cast", grids, S, tfd, A, o, d, R, _lib.LEAF_MODES[mode], *args, *out,
                      f64=dtype == torch.float64)
        # leaves return on their own device (sdf.py:546)
        return _ray_result(out, batch + lead, self.sdfs[0].device), {"o": o, "d": d, "out": out, "tfd": tfd, "grids": grids,
                                                                      "S": S, "A": A, "mode": mode}

    def _ray_cast_per_configuration(self, o, d, lead, dtype, args, batch, graph=None):
        """Compositions the kernel does not serve (other leaves, mixed modes, non-rigid transforms, other dtypes): the torch loop
        around __call__ for each configuration's own composition -- not a hot path.  graph (_ray_graph): the rays get the
        gradient of the hit distance, summed over the configurations by torch; transforms that require grad raise, since their
        gradient would be dropped without a word."""
        if graph is not None and self._tf_grad:
            raise ValueError("ray_cast(differentiable=True): this composition is not served by the fused kernels (mixed or generic "
                             "leaves, non-rigid transforms or another dtype), so its transforms get no gradient; detach them or "
                             "use a fused composition")
        S, A = len(self.sdfs), math.prod(batch)
        stack = self._tf_matrix.detach().reshape(S, A, 4, 4)
        rows = []
        for a in range(A):
            one = ComposedSDF(self.sdfs, None)
            one.set_transforms(stack[:, a], known_rigid=self._rigid)
            rows.append(one._ray_cast_generic(o, d, lead, dtype, args, graph))
        if not rows:
            dev = o.device if o.device.type != "cpu" else d.device
            return _ray_result(_ray_outputs(batch + lead, dtype, dev), batch + lead, dev)
        return RayCast(*(torch.stack(x).reshape(*batch, *x[0].shape) for x in zip(*rows)))

    # ---- hinge penalty over points ----
    def hinge_over_points(self, points, margin, power=2, per_leaf=False):
        """The clearance cost of an SDF-based trajectory optimiser, ((margin - v).clamp(min=0) ** power).sum over the points, for
        every configuration, without the (A, P) field.

        :param points: (..., 3); the leading dimensions are flattened into P
        :param margin: a finite Python real number, rounded once to the query dtype (torch's rule for a scalar against a tensor)
        :param power: 1 or 2
        :param per_leaf: False: the hinge of the composed value (what __call__ returns); True: one hinge per leaf s
            (leaf s = self.sdfs[s], alone under its own transforms)
        :return: HingeOverPoints(values, counts) of shape B (per_leaf: B + (S,)), B the transform batch shape (() without one).
            values have the dtype __call__ returns: each term is rounded in that dtype exactly as the torch expression rounds it,
            and the terms are summed in float64 in a fixed order that depends only on (S, A, P), then rounded once (float32:
            within 1 ulp of the exactly rounded sum; two calls give the same bits).  A NaN value makes its row NaN, as
            torch.sum does.  counts are int64: the number of points with v < margin (a NaN is not counted).  No points give
            zeros.  Differentiable w.r.t. the points and the transforms (a RobotSDF's joint values) when grad mode is on and
            they require grad: the gradient torch autograd gives through ((margin - __call__(points)[0]).clamp(min=0) **
            power).sum(-1) with the forward's decisions held fixed (clamp passes the gradient at v == margin; a nearest leaf in
            range has no derivative w.r.t. the point); counts carry no gradient.  Gradients need at most 64 leaves;
            create_graph=True raises.

        Fused compositions (_fused_mode(): every leaf a BOUNDING_BOX CachedSDF of one interpolation, rigid transforms) with float32
        or float64 points run HIP kernels (csrc/hinge_over_points.hip, and the backward in csrc/backward.hip) with extra memory
        O(A Z P / 4096) (Z = 1, or S per leaf) and nothing that synchronises with the host, so the call can be captured in a
        graph; anything else is __call__ plus the torch expression, summed in float64, under the same contract (differentiable
        wherever __call__ is)."""
        if not isinstance(per_leaf, bool):
            raise TypeError(f"per_leaf must be True or False, got {per_leaf!r}")
        margin, power = _hinge_args(margin, power)
        if not torch.is_tensor(points):
            points = torch.as_tensor(points)
        if points.dim() < 1 or points.shape[-1] != 3:
            raise ValueError(f"query points must have last dimension 3, got {tuple(points.shape)}")
        if self._tf_matrix is None:
            raise ValueError("hinge_over_points needs the transforms to be set")
        mode = self._fused_mode()
        fused = mode is not None and points.dtype in (torch.float32, torch.float64)
        if points.numel() == 0:  # torch's empty sum: zeros, nothing launched
            batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
            shape = batch + ((len(self.sdfs),) if per_leaf else ())
            dtype = points.dtype if points.dtype == torch.float64 or not fused else torch.float32
            if not dtype.is_floating_point:
                dtype = torch.get_default_dtype()
            dev = getattr(self.sdfs[0], "device", self._tf_matrix.device)
            return HingeOverPoints(torch.zeros(shape, dtype=dtype, device=dev), torch.zeros(shape, dtype=torch.int64, device=dev))
        if not fused:
            return self._hinge_over_points_generic(points, margin, power, per_leaf)
        if (self._tf_grad or points.requires_grad) and torch.is_grad_enabled():
            from pytorch_volumetric_amd import autograd
            return autograd.hinge_over_points(self, points, margin, power, mode, per_leaf)
        val, cnt = self._hinge_over_points_fused(points, margin, power, mode, per_leaf)[:2]
        return HingeOverPoints(val, cnt)

    def _hinge_over_points_fused(self, points, margin, power, mode, per_leaf):
        """One pvamd_composed_hinge_over_points[_f64] call.  Returns (values, counts) in the result shapes on the leaves' device,
        then what the backward needs: the flat points and the stack the kernels read."""
        S = len(self.sdfs)
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        A = math.prod(batch)
        dev = self._owner_device()
        flat, tfd, dtype = self._fused_inputs(points, dev)
        P, Z = flat.shape[0], S if per_leaf else 1
        val = torch.empty((A, Z), dtype=flat.dtype, device=dev)
        cnt = torch.empty((A, Z), dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            scratch = _lib.scratch_buffer(_lib.hinge_over_points_scratch_bytes(S, A, P, per_leaf), dev)
            _lib.call("pvamd_composed_hinge_over_points", grids, S, tfd, A, flat, P, _lib.LEAF_MODES[mode], per_leaf, margin, power,
                      val, cnt, scratch, f64=flat.dtype == torch.float64)
        shape = batch + ((S,) if per_leaf else ())
        out_device = self.sdfs[0].device  # leaves return on their own device (sdf.py:546)
        return val.reshape(shape).to(device=out_device, dtype=dtype), cnt.reshape(shape).to(device=out_device), flat, tfd

    def _hinge_over_points_generic(self, points, margin, power, per_leaf):
        """Compositions the kernels do not serve (other leaves, mixed modes, other dtypes): __call__ (per leaf: the one-leaf
        composition) and the torch expression, summed in float64 -- not a hot path.  Differentiable through __call__."""
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        if per_leaf:
            parts = []
            for s in range(len(self.sdfs)):
                one = ComposedSDF([self.sdfs[s]], None)
                one.set_transforms(self._tf_matrix[self.ith_transform_slice(s)], batch_dim=self.tsf_batch,
                                   known_rigid=self._rigid)
                parts.append(one._hinge_over_points_generic(points, margin, power, False))
            return HingeOverPoints(*(torch.stack(t, dim=len(batch)) for t in zip(*parts)))
        A = math.prod(batch)
        val = self(points)[0].reshape(A, -1)
        terms = (margin - val).clamp(min=0) ** power
        values = terms.to(torch.float64).sum(-1).to(val.dtype)
        counts = (val.detach() < margin).sum(-1)
        return HingeOverPoints(values.reshape(batch), counts.reshape(batch))

    # ---- leaf-pair distance ----
    def _pair_device(self):
        """The GPU the pair kernels run on: the leaves' own for fused compositions, else the current one."""
        return self._owner_device() if self._fused_mode() is not None else _lib.require_gpu()

    def _pairs_host(self, pairs):
        """pairs -> (K, 2) int64 CPU tensor, validated against the leaf count (a device tensor is read once)."""
        S = len(self.sdfs)
        p = pairs if torch.is_tensor(pairs) else torch.as_tensor(pairs, dtype=torch.int64)
        if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool:
            raise ValueError(f"pairs must be integers, got {p.dtype}")
        if p.numel() == 0:
            p = p.reshape(0, 2)
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError(f"pairs must have shape (K, 2), got {tuple(p.shape)}")
        p = p.detach().to(device="cpu", dtype=torch.int64)
        if p.numel():
            if int(p.min()) < 0 or int(p.max()) >= S:
                raise ValueError(f"pair index out of range for {S} leaves")
            if bool((p[:, 0] == p[:, 1]).any()):
                raise ValueError("a pair (s, t) needs s != t")
        return p

    def _stack_for(self, dtype, dev):
        """The (S*A, 4, 4) stack the pair kernels read: float32, or the exact float64 widening of what __call__ reads."""
        if dtype == torch.float64:
            tfd = self.__dict__.get("_tf_dev64")
            if tfd is None or tfd.device != dev:
                tfd = self._tf_dev64 = self._tf_matrix.detach().to(device=dev, dtype=torch.float64).contiguous()
            return tfd
        return self._tf_device(dev)

    def _leaf_pair_plan(self, leaf_points, pairs):
        """Validated pairs, the device pair table (s, t, offset, P_t) and the packed points, built once per (pairs, points) and
        kept while the caller passes the same unmodified tensors (the cache holds them, so their ids cannot be re-used)."""
        S = len(self.sdfs)
        if isinstance(leaf_points, torch.Tensor) or len(leaf_points) != S:
            raise ValueError(f"leaf_points must be a sequence of {S} point sets, one per leaf")
        inputs = (pairs, *leaf_points)
        key = tuple((x.data_ptr(), x._version, tuple(x.shape), x.dtype, str(x.device)) if torch.is_tensor(x) else None
                    for x in inputs)
        hit = self.__dict__.get("_pair_plan")
        if hit is not None and None not in key and len(hit[0]) == len(inputs) and \
                all(a is b for a, b in zip(hit[0], inputs)) and hit[1] == key:
            return hit[2]
        ph = self._pairs_host(pairs)
        pts = [p if torch.is_tensor(p) else torch.as_tensor(p) for p in leaf_points]
        for i, p in enumerate(pts):
            if p.dim() < 1 or p.shape[-1] != 3:
                raise ValueError(f"leaf_points[{i}] must have last dimension 3, got {tuple(p.shape)}")
        counts = [p.numel() // 3 for p in pts]
        for t in ph[:, 1].tolist():
            if counts[t] == 0:
                raise ValueError(f"leaf_points[{t}] is empty but a pair uses it as its point side")
        qdtype = torch.float64 if any(p.dtype == torch.float64 for p in pts) else torch.float32
        if ph.shape[0] == 0:  # nothing to pack or launch
            dev = getattr(self.sdfs[0], "device", None) or self._tf_matrix.device
            return dict(pairs=ph, dtype=qdtype, dev=torch.device(dev))
        dev = self._pair_device()
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + c)
        packed = torch.cat([p.detach().reshape(-1, 3).to(device=dev, dtype=qdtype) for p in pts]).contiguous()
        table = torch.tensor([[s, t, offs[t], counts[t]] for s, t in ph.tolist()], dtype=torch.int64).reshape(-1, 4).to(dev)
        max_points = max((counts[t] for t in ph[:, 1].tolist()), default=0)
        plan = dict(pairs=ph, table=table, packed=packed, npoints=offs[-1], max_points=max_points, dtype=qdtype, dev=dev,
                    points=pts)
        if None not in key:
            self._pair_plan = (inputs, key, plan)
        return plan

    def _pair_transforms(self, table, K, dtype, dev):
        """pvamd_leaf_pair_transforms[_f64]: (K, A, 4, 4) in dtype on dev, from the stack the kernels read."""
        S = len(self.sdfs)
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        tfd = self._stack_for(dtype, dev)
        C = torch.empty((K, A, 4, 4), dtype=dtype, device=dev)
        if K:
            with _lib.on_device(dev):
                _lib.call("pvamd_leaf_pair_transforms", tfd, S, A, table, K, C, f64=dtype == torch.float64)
        return C, tfd

    def leaf_pair_transforms(self, pairs, dtype=torch.float32):
        """The leaf t frame -> leaf s frame transforms of the ordered pairs (s, t): C = Ms Mt^-1 with the rigid inverse, the exact
        bits leaf_pair_distance uses (include/pvamd.h "Leaf-pair distance" 1).

        :param pairs: int (K, 2) ordered leaf pairs (s, t), s != t
        :param dtype: torch.float32 or torch.float64 (the float64 stack is the exact widening of the float32 one)
        :return: B + (K, 4, 4), B the transform batch shape (() without one).  Not differentiable."""
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        self._check_pair_transforms()
        ph = self._pairs_host(pairs)
        K = ph.shape[0]
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        if K == 0:
            return torch.empty(batch + (0, 4, 4), dtype=dtype, device=self._tf_matrix.device)
        dev = self._pair_device()
        table = torch.cat((ph, torch.zeros_like(ph)), dim=1).to(dev)
        C, _ = self._pair_transforms(table, K, dtype, dev)
        return C.transpose(0, 1).reshape(*batch, K, 4, 4)

    def _check_pair_transforms(self):
        if self._tf_matrix is None:
            raise ValueError("leaf-pair queries need the transforms to be set")
        if not self._rigid:
            raise ValueError("leaf-pair queries need rigid transforms (the pair transform inverts each leaf transform as a rigid one)")

    def leaf_pair_distance(self, leaf_points, pairs):
        """For every configuration and ordered pair (s, t): the point of leaf t's set where leaf s's SDF is smallest -- how
        close leaf t comes to leaf s -- without an (A, K, P) buffer.

        :param leaf_points: a sequence of S point sets (P_s, 3), each in its own leaf's frame (leaf s = self.sdfs[s], the frame
            its SDF is queried in).  A set may be empty only if no pair uses it as its point side.  float64 results when any set
            is float64 (the others are widened exactly), float32 otherwise.
        :param pairs: int (K, 2) ordered pairs (s, t), s != t: the points of leaf t against the SDF of leaf s.  The two directions
            are different queries; torch.minimum of the two gives the symmetric distance.
        :return: LeafPairDistance(values, indices, gradients) of shapes B + (K,), B + (K,), B + (K, 3), B the transform batch
            shape (() without one).  Per (configuration, pair) the bits ComposedSDF([sdfs[s]], C[:, k]).min_over_points(
            leaf_points[t]) returns, C = leaf_pair_transforms(pairs) in the result dtype: indices (int64) index leaf_points[t]
            (ties to the smallest index, a NaN counts as the minimum, -0.0 and +0.0 tie); gradients are leaf s's SDF gradient at
            the witness point rotated back by C, so they are expressed in LEAF t's FRAME.  Differentiable w.r.t. the transforms
            (a RobotSDF's joint values) when grad mode is on and they require grad, decisions held fixed; the points carry no
            gradient.  Gradients need at most 64 leaves; create_graph=True raises.

        Fused compositions (_fused_mode(): every leaf a BOUNDING_BOX CachedSDF of one interpolation) run HIP kernels
        (csrc/leaf_pair.hip) with extra memory O(A K chunks) and nothing that synchronises with the host once the pair table
        is built (it is kept while the same pairs and point tensors are passed), so the call can be captured in a graph.  Any
        other composition takes the pair transforms from the same kernel and runs one one-leaf min_over_points per pair
        (differentiable wherever __call__ is)."""
        self._check_pair_transforms()
        plan = self._leaf_pair_plan(leaf_points, pairs)
        K = plan["pairs"].shape[0]
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        mode = self._fused_mode()
        if K == 0:
            dev, dt = plan["dev"], plan["dtype"]
            return LeafPairDistance(torch.empty(batch + (0,), dtype=dt, device=dev),
                                    torch.empty(batch + (0,), dtype=torch.int64, device=dev),
                                    torch.empty(batch + (0, 3), dtype=dt, device=dev))
        if mode is None:
            return self._leaf_pair_generic(plan)
        if self._tf_grad and torch.is_grad_enabled():
            from pytorch_volumetric_amd import autograd
            return autograd.leaf_pair_distance(self, plan, mode)
        return LeafPairDistance(*self._leaf_pair_fused(plan, mode)[:3])

    def _leaf_pair_fused(self, plan, mode):
        """pvamd_leaf_pair_transforms + pvamd_leaf_pair_distance[_f64].  Returns (values, indices, gradients) in the result shapes,
        then what the backward needs: the (A, K) indices, the pair transforms and the stack the kernels read."""
        S = len(self.sdfs)
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        A = math.prod(batch)
        dev, dt, table = plan["dev"], plan["dtype"], plan["table"]
        K = table.shape[0]
        C, tfd = self._pair_transforms(table, K, dt, dev)
        val = torch.empty((A, K), dtype=dt, device=dev)
        grad = torch.empty((A, K, 3), dtype=dt, device=dev)
        idx = torch.empty((A, K), dtype=torch.int64, device=dev)
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            n = _lib.leaf_pair_scratch_bytes(K, A, plan["max_points"], f64, False)
            scratch = _lib.scratch_buffer(n, dev) if n else None
            _lib.call("pvamd_leaf_pair_distance", grids, S, C, A, plan["packed"], plan["npoints"], table, K, plan["max_points"],
                      _lib.LEAF_MODES[mode], val, grad, idx, scratch, f64=f64)
        return val.reshape(*batch, K), idx.reshape(*batch, K), grad.reshape(*batch, K, 3), idx, C, tfd

    def _leaf_pair_generic(self, plan):
        """Compositions the kernels do not serve (MeshSDF leaves, mixed interpolation, other leaves): the pair transforms of the
        kernel, then one one-leaf min_over_points per pair -- not a hot path.  Differentiable through __call__, and to the
        transforms through autograd.PairTransforms."""
        from pytorch_volumetric_amd import autograd
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        ph = plan["pairs"]
        C = autograd.pair_transforms(self, plan["table"], ph, plan["dtype"], plan["dev"])  # (K, A, 4, 4)
        parts = []
        for k, (s, t) in enumerate(ph.tolist()):
            one = ComposedSDF([self.sdfs[s]], None)
            one.set_transforms(C[k], batch_dim=self.tsf_batch, known_rigid=True)
            pts = plan["points"][t]
            parts.append(one.min_over_points(pts.to(plan["dtype"]) if pts.dtype != plan["dtype"] else pts))
        return LeafPairDistance(*(torch.stack(x, dim=len(batch)) for x in zip(*parts)))

    # ---- leaf-pair hinge ----
    def leaf_pair_hinge(self, leaf_points, pairs, margin, power=2):
        """For every configuration and ordered pair (s, t): the self-collision cost of leaf t's points against leaf s's SDF,
        sum_p max(margin - v, 0) ** power, and the number of those points with v < margin -- the hinge sum a CHOMP, TrajOpt
        or MPPI cost needs, without an (A, K, P) buffer.

        :param leaf_points: as for leaf_pair_distance: S point sets (P_s, 3), each in its own leaf's frame; a set may be empty
            only if no pair uses it as its point side; float64 results when any set is float64
        :param pairs: as for leaf_pair_distance: int (K, 2) ordered pairs (s, t), s != t (points of leaf t, SDF of leaf s)
        :param margin: a finite Python real number, rounded once to the result dtype
        :param power: 1 or 2
        :return: LeafPairHinge(values, counts), both of shape B + (K,), B the transform batch shape (() without one); counts
            are int64.  Per (configuration, pair) the bits ComposedSDF([sdfs[s]], C[:, k]).hinge_over_points(leaf_points[t],
            margin, power) returns, C = leaf_pair_transforms(pairs) in the result dtype: each term rounded as torch rounds
            (margin - v).clamp(min=0) ** power, summed in float64 in that call's fixed order and rounded once; a NaN v makes
            its value NaN and is not counted.  Differentiable w.r.t. the transforms (a RobotSDF's joint values) when grad mode
            is on and they require grad, decisions held fixed (clamp passes the gradient at v == margin); the points carry no
            gradient.  As for hinge_over_points, a point inside leaf s's grid range has no derivative with nearest leaves:
            only points in the bounding-box branch move the transforms; trilinear leaves (cache_link_sdf_factory(...,
            interpolation="trilinear")) give a gradient everywhere in range.  Gradients need at most 64 leaves;
            create_graph=True raises.

        Fused compositions (_fused_mode(): every leaf a BOUNDING_BOX CachedSDF of one interpolation) run HIP kernels
        (csrc/leaf_pair.hip) with extra memory O(A K chunks) and nothing that synchronises with the host once the pair table
        is built, so the call can be captured in a graph.  Any other composition takes the pair transforms from the same
        kernel and runs one one-leaf hinge_over_points per pair (differentiable wherever __call__ is)."""
        margin, power = _hinge_args(margin, power)
        self._check_pair_transforms()
        plan = self._leaf_pair_plan(leaf_points, pairs)
        K = plan["pairs"].shape[0]
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        if K == 0:
            dev, dt = plan["dev"], plan["dtype"]
            return LeafPairHinge(torch.empty(batch + (0,), dtype=dt, device=dev),
                                 torch.empty(batch + (0,), dtype=torch.int64, device=dev))
        mode = self._fused_mode()
        if mode is None:
            return self._leaf_pair_hinge_generic(plan, margin, power)
        if self._tf_grad and torch.is_grad_enabled():
            from pytorch_volumetric_amd import autograd
            return autograd.leaf_pair_hinge(self, plan, margin, power, mode)
        return LeafPairHinge(*self._leaf_pair_hinge_fused(plan, margin, power, mode)[:2])

    def _leaf_pair_hinge_fused(self, plan, margin, power, mode):
        """pvamd_leaf_pair_transforms + pvamd_leaf_pair_hinge[_f64].  Returns (values, counts) in the result shapes, then what
        the backward needs: the pair transforms and the stack the kernels read."""
        S = len(self.sdfs)
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        A = math.prod(batch)
        dev, dt, table = plan["dev"], plan["dtype"], plan["table"]
        K = table.shape[0]
        C, tfd = self._pair_transforms(table, K, dt, dev)
        val = torch.empty((A, K), dtype=dt, device=dev)
        cnt = torch.empty((A, K), dtype=torch.int64, device=dev)
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            n = _lib.leaf_pair_hinge_scratch_bytes(K, A, plan["max_points"], f64, False)
            scratch = _lib.scratch_buffer(n, dev) if n else None
            _lib.call("pvamd_leaf_pair_hinge", grids, S, C, A, plan["packed"], plan["npoints"], table, K, plan["max_points"],
                      _lib.LEAF_MODES[mode], margin, power, val, cnt, scratch, f64=f64)
        return val.reshape(*batch, K), cnt.reshape(*batch, K), C, tfd

    def _leaf_pair_hinge_generic(self, plan, margin, power):
        """Compositions the kernels do not serve (MeshSDF leaves, mixed interpolation, other leaves): the pair transforms of the
        kernel, then one one-leaf hinge_over_points per pair -- not a hot path.  Differentiable through __call__, and to the
        transforms through autograd.PairTransforms."""
        from pytorch_volumetric_amd import autograd
        batch = tuple(self.tsf_batch) if self.tsf_batch is not None else ()
        ph = plan["pairs"]
        C = autograd.pair_transforms(self, plan["table"], ph, plan["dtype"], plan["dev"])  # (K, A, 4, 4)
        parts = []
        for k, (s, t) in enumerate(ph.tolist()):
            one = ComposedSDF([self.sdfs[s]], None)
            one.set_transforms(C[k], batch_dim=self.tsf_batch, known_rigid=True)
            pts = plan["points"][t]
            parts.append(one.hinge_over_points(pts.to(plan["dtype"]) if pts.dtype != plan["dtype"] else pts, margin, power))
        return LeafPairHinge(*(torch.stack(x, dim=len(batch)) for x in zip(*parts)))

    def _interp_forward(self, points, want_leaf):
        """_fused_forward of a trilinear composition (the leaf ids the interpolation tests compare)."""
        return self._fused_forward(points, "trilinear", want_leaf=want_leaf)

    # ---- prepared point sets: a planner that queries the SAME points under many configurations, step after step ----
    def prepare_points(self, points_in_object_frame):
        """Sort a point set along the Hilbert curve ONCE and keep the order: a handle for query_prepared().  The drop-in call
        (__call__ with README-size leaf grids) pays this sort and an un-permute pass on every call (model_to_sdf.py:117-125
        re-queried per joint configuration, README.md:150-200); a planner that re-uses its query points -- a fixed workspace
        grid, a fixed set of collision spheres -- pays the sort here and, with order="sorted", nothing per call.
        `points_in_object_frame`: [...] x N x 3, any float dtype / device (computed in float32 on the leaves' GPU)."""
        _require_nearest(self, "prepare_points")
        if not self._fusable():
            raise ValueError("prepare_points needs every leaf to be a CachedSDF with the BOUNDING_BOX strategy")
        if not torch.is_tensor(points_in_object_frame):
            points_in_object_frame = torch.as_tensor(points_in_object_frame)
        flat, lead, dtype, device = _lib.as_query_points(points_in_object_frame, self._owner_device())
        P = flat.shape[0]
        if P == 0:
            raise ValueError("prepare_points needs at least one point")
        with _lib.on_device(flat.device):
            order, inv, spts = _lib.morton_order(flat, min_points=0, want_inverse=True, want_sorted=True)
            Pp = _lib.whole_tiles(P)
            padded = spts if Pp == P else torch.cat((spts, spts[-1:].expand(Pp - P, 3))).contiguous()
        return PreparedPoints(flat, order, inv, spts, padded, tuple(lead), dtype)

    def query_prepared(self, prepared: "PreparedPoints", order="caller"):
        """The fused query over a prepare_points() handle under the CURRENT transforms (set_transforms /
        RobotSDF.set_joint_configuration between calls as usual).
        order="caller": exactly what __call__(points) returns -- same shapes, same bits -- without the per-call sort (for float32
            and lower-precision points; float64 points were rounded to float32 by prepare_points, whereas __call__ answers
            them with float64 index arithmetic, sdf.py:545: prepare float32 points if the two must agree).
        order="sorted": (A..., P) / (A..., P, 3) with column j the result of caller point `prepared.order[j]` (flattened
        index): no sort and no un-permute pass -- the kernel's own output order.  Same bits, permuted."""
        if order not in ("caller", "sorted"):
            raise ValueError('order must be "caller" or "sorted"')
        _require_nearest(self, "query_prepared")
        if not self._fusable():
            raise ValueError("query_prepared needs every leaf to be a CachedSDF with the BOUNDING_BOX strategy")
        S = len(self.sdfs)
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        dev = self._owner_device()
        if prepared.points.device != dev:
            raise _lib.PvamdError(f"query_prepared: the leaf grids live on {dev}; the prepared points are on {prepared.points.device}")
        P = prepared.points.shape[0]
        val = torch.empty((A, P), dtype=torch.float32, device=dev)
        grad = torch.empty((A, P, 3), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            tfd = self._tf_device(dev)
            if order == "sorted":
                # (already sorted along the Hilbert curve: regrouping inside chunks would only cost its sort)
                _lib.call("pvamd_composed_query", grids, S, tfd, A, prepared.sorted_points, P, val, grad, None,
                          self._query_flags | _lib.COMPOSED_NO_GROUPING)
            else:
                Pp = prepared.padded_points.shape[0]
                scratch = torch.empty((A, Pp, 4), dtype=torch.float32, device=dev)
                _lib.call("pvamd_composed_query_bucketed", grids, S, tfd, A, prepared.padded_points, prepared.inverse, P, Pp,
                          scratch, val, grad, self._query_flags)
        lead = (P,) if order == "sorted" else prepared.lead
        out_device = self.sdfs[0].device
        if self.tsf_batch is not None:
            val, grad = val.reshape(*self.tsf_batch, *lead), grad.reshape(*self.tsf_batch, *lead, 3)
        else:
            val, grad = val.reshape(-1), grad.reshape(-1, 3)  # like __call__: flat without a transform batch (sdf.py:433)
        return val.to(device=out_device, dtype=prepared.dtype), grad.to(device=out_device, dtype=prepared.dtype)

    def query_packed(self, points, out=None):
        """Fused query that leaves one (val, gx, gy, gz) record per (configuration, point): (A, P, 4) fp32 for contiguous
        fp32 (P, 3) GPU points, P a multiple of _lib.TILE_POINTS.  What a query sharded over GPUs gathers (one buffer instead of two,
        unpacked straight into the final layout: dist.ShardedSDF); same bits as __call__."""
        _require_nearest(self, "query_packed")
        if not self._fusable():
            raise ValueError("query_packed needs every leaf to be a CachedSDF with the BOUNDING_BOX strategy")
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        P = points.shape[0]
        if not (points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and points.shape == (P, 3)) \
                or P % _TILE_POINTS != 0 or P == 0:
            raise ValueError(f"query_packed needs contiguous fp32 (P,3) points on the GPU, P a positive multiple of {_TILE_POINTS}")
        dev = points.device
        if dev != self._owner_device():
            raise _lib.PvamdError(f"query_packed: the leaf grids live on {self._owner_device()}; points are on {dev}")
        if out is None:
            out = torch.empty((A, P, 4), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            if self._grouping_pays(A, P, self._query_flags):
                scratch = _lib.group_points(points)
                _lib.call("pvamd_composed_query_grouped", grids, len(self.sdfs), self._tf_device(dev), A, scratch, P, out, None, None,
                          self._query_flags | _lib.COMPOSED_OUT_PACKED)
                return out
            _lib.call("pvamd_composed_query_packed", grids, len(self.sdfs), self._tf_device(dev), A, points, P, out,
                      self._query_flags)
        return out

    def query_configs(self, points, first, count):
        """The fused query for configurations [first, first + count) of the flattened batch only (indices past the last
        configuration repeat it): fp32 (count, P) / (count, P, 3) on the leaves' GPU.  What a query sharded over
        configurations runs on each rank (dist.ShardedSDF(shard="configs")); same bits as the rows of __call__."""
        _require_nearest(self, "query_configs")
        if not self._fusable() or self.tsf_batch is None:
            raise ValueError("query_configs needs BOUNDING_BOX CachedSDF leaves and a configuration batch")
        S, A = len(self.sdfs), math.prod(self.tsf_batch)
        dev = self._owner_device()
        pick = torch.arange(first, first + count, device=dev).clamp_max(A - 1)
        if torch.is_tensor(points) and points.dtype == torch.float64:
            # float64 query points stay float64 (sdf.py:395-431 over sdf.py:545-547), as in __call__
            val, grad, _, _, _ = self._fused_forward(points, "nearest", configs=pick)
            return val, grad
        flat, _, _, _ = _lib.as_query_points(points, dev)
        P = flat.shape[0]
        sub = self._tf_device(dev).reshape(S, A, 4, 4)[:, pick].contiguous()
        val = torch.empty((count, P), dtype=torch.float32, device=dev)
        grad = torch.empty((count, P, 3), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            _lib.call("pvamd_composed_query", grids, S, sub, count, flat, P, val, grad, None, self._direct_flags())
        return val, grad

    def query_into(self, points, out_val, out_grad):
        """Allocation-free fused query for inner loops / graph capture: contiguous fp32 (P,3) GPU points, results into
        the caller's fp32 (A,P) / (A,P,3) buffers (A = number of configurations, 1 without a transform batch).  Needs
        every leaf to be a BOUNDING_BOX CachedSDF.  One C-ABI call, one kernel launch on the current stream (two of each where
        the chunk-grouped kernel pays: `group_points`)."""
        _require_nearest(self, "query_into")
        if not self._fusable():
            raise ValueError("query_into needs every leaf to be a CachedSDF with the BOUNDING_BOX strategy")
        A = math.prod(self.tsf_batch) if self.tsf_batch is not None else 1
        P = points.shape[0]
        if not (points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and points.shape == (P, 3)):
            raise ValueError("query_into needs contiguous fp32 (P,3) points on the GPU")
        if out_val.numel() != A * P or out_grad.numel() != 3 * A * P or out_val.dtype != torch.float32 or \
                out_grad.dtype != torch.float32 or not (out_val.is_contiguous() and out_grad.is_contiguous()):
            raise ValueError("query_into needs contiguous fp32 outputs with A*P and A*P*3 elements")
        dev = points.device
        if not (dev == self._owner_device() == out_val.device == out_grad.device):
            raise _lib.PvamdError(f"query_into: the leaf grids live on {self._owner_device()}; points / outputs are on "
                                  f"{dev} / {out_val.device} / {out_grad.device}")
        with _lib.on_device(dev):
            grids = self._leaf_grids(dev)
            if self._grouping_pays(A, P, self._query_flags):
                # two launches (the chunk sort, the query) over a scratch buffer this object keeps per point count: nothing is
                # allocated after the first call of a size, so a captured graph replays both
                need = int(_lib.load().pvamd_group_scratch_bytes(P))
                # one buffer per (point count, device, stream): two streams querying the same object never share a scratch.
                # At most 8 are remembered -- except those a stream capture has seen: a captured graph replays with the
                # buffer's address, so such a buffer lives as long as this object
                table = self.__dict__.setdefault("_group_scratch", {})
                key = (need, str(dev), _lib.stream_ptr().value or 0)
                entry = table.get(key)
                if entry is None:
                    loose = [k for k, e in table.items() if not e[1]]
                    if len(loose) >= 8:
                        table.pop(loose[0])
                    entry = table[key] = [torch.empty((need,), dtype=torch.uint8, device=dev), False]
                if not entry[1] and torch.cuda.is_current_stream_capturing():
                    entry[1] = True
                scratch = entry[0]
                _lib.call("pvamd_group_points", points, P, scratch)
                _lib.call("pvamd_composed_query_grouped", grids, len(self.sdfs), self._tf_device(dev), A, scratch, P,
                          out_val, out_grad, None, self._query_flags)
                return
            _lib.call("pvamd_composed_query", grids, len(self.sdfs), self._tf_device(dev), A, points, P, out_val, out_grad, None,
                      self._direct_flags())

    def _generic_f64(self, points, S, A):
        """float64 query points over leaves that are not cached grids: sdf.py:395-431 runs transform_points, transform_normals
        and the argmin in the query dtype, and every leaf is asked with the float64 image of the points (a MeshSDF leaf rounds
        that image to float32 itself, sdf.py:132 -- ONE rounding, of the float64 result, where transforming in float32 rounds
        every product).  Plain torch on the GPU: this is the reference's own dtype path, not a hot one; results in float64."""
        dev = _lib.require_gpu()
        pts_shape = points.shape
        flat = points.detach().reshape(-1, 3).to(device=dev, dtype=torch.float64)
        P = flat.shape[0]
        m = self._tf_matrix.to(device=dev, dtype=torch.float64).reshape(S, A, 4, 4)
        best_v = best_g = None
        for i, sdf in enumerate(self.sdfs):
            M = m[i]  # (A, 4, 4) object frame -> leaf frame
            # separate, unfused float64 operations in a fixed order (the test restates them in numpy)
            x = [M[:, r, 0, None] * flat[None, :, 0] + M[:, r, 1, None] * flat[None, :, 1] + M[:, r, 2, None] * flat[None, :, 2]
                 + M[:, r, 3, None] for r in range(3)]
            v, g = sdf(torch.stack(x, dim=-1))  # (A, P), (A, P, 3) in the leaf frame
            v = v.to(device=dev, dtype=torch.float64).reshape(A, P)
            g = g.to(device=dev, dtype=torch.float64).reshape(A, P, 3)
            # back to the object frame with R^T of the (rigid) object -> leaf rotation (sdf.py:409)
            g = torch.stack([M[:, 0, j, None] * g[..., 0] + M[:, 1, j, None] * g[..., 1] + M[:, 2, j, None] * g[..., 2]
                             for j in range(3)], dim=-1)
            if best_v is None:
                best_v, best_g = v, g
            else:  # torch.argmin (sdf.py:421): the first minimum wins, a NaN counts as the minimum
                take = (v < best_v) | (torch.isnan(v) & ~torch.isnan(best_v))
                best_v = torch.where(take, v, best_v)
                best_g = torch.where(take.unsqueeze(-1), g, best_g)
        if self.tsf_batch is not None:
            best_v = best_v.reshape(*self.tsf_batch, *pts_shape[:-1])
            best_g = best_g.reshape(*self.tsf_batch, *pts_shape[:-1], 3)
        else:
            best_v, best_g = best_v.reshape(-1), best_g.reshape(-1, 3)
        return best_v.to(points.device), best_g.to(points.device)

    def _generic(self, flat, S, A):
        """Leaves that are not cached grids (MeshSDF -- the reference's own tests/test_sdf.py:61-80 -- SphereSDF, nested
        compositions): per leaf one transform kernel, the leaf's own query, one merge kernel (pvamd_transform_points /
        pvamd_compose_merge: the fused kernel's arithmetic, valid for any affine transform)."""
        dev = flat.device
        P = flat.shape[0]
        m = self._tf_device(dev).reshape(S, A, 4, 4)
        best_v = torch.empty((A, P), dtype=torch.float32, device=dev)
        best_g = torch.empty((A, P, 3), dtype=torch.float32, device=dev)
        # MeshSDF leaves want their points in a spatial order; every leaf sees a rigid image of the SAME points, so ONE spatial
        # order of the object-frame points (repeated per configuration) serves all of them instead of a sort per leaf
        order = None
        if any(isinstance(s, MeshSDF) for s in self.sdfs) and getattr(self, "_rigid", True) and A * P < 2 ** 31:
            with _lib.on_device(dev):
                order = _lib.morton_order(flat)  # None for a handful of points: the leaves then sort for themselves
            if order is not None and A > 1:
                order = (order.unsqueeze(0) + (torch.arange(A, device=dev, dtype=torch.int32) * P).unsqueeze(1)).reshape(-1)
        x = torch.empty((A, P, 3), dtype=torch.float32, device=dev)
        for i, sdf in enumerate(self.sdfs):
            with _lib.on_device(dev):
                _lib.call("pvamd_transform_points", m[i], A, flat, P, x)
            if order is not None and isinstance(sdf, MeshSDF):
                res = sdf.obj_factory.object_frame_closest_point(x, order=order)
                v, g = res.distance, res.gradient
            else:
                v, g = sdf(x)
            v = v.to(device=dev, dtype=torch.float32).reshape(A, P).contiguous()
            g = g.to(device=dev, dtype=torch.float32).reshape(A, P, 3).contiguous()
            with _lib.on_device(dev):
                _lib.call("pvamd_compose_merge", m[i], A, P, v, g, i, i == 0, best_v, best_g, None)
        return best_v, best_g


def sample_mesh_points(obj_factory: ObjectFactory = None, num_points=100, seed=0, name="",
                       clean_cache=False, dtype=torch.float, min_init_sample_points=200,
                       dbpath='model_points_cache.pkl', device="cpu", cache=None):
    """Seeded area-uniform surface samples + face normals (role of sdf.py:617-670).

    The reference draws these from open3d's RNG, which cannot be reproduced; this sampler keeps the call signature,
    the over-sample-then-subselect scheme, the normals from the mesh query, the return triple and the cache layout
    (cache[name][seed][num_points] = (points, normals, None)), with a counter-based draw on the GPU."""
    given_cache = cache is not None
    if cache is not None or (dbpath is not None and os.path.exists(dbpath)):
        if cache is None:
            cache = torch.load(dbpath, weights_only=False)
        cache.setdefault(name, {}).setdefault(seed, {})
        if not clean_cache and num_points in cache[name][seed]:
            res = cache[name][seed][num_points]
            res = list(v.to(device=device, dtype=dtype) if v is not None else None for v in res)
            return *res[:-1], cache
    else:
        cache = {name: {seed: {}}}
    if obj_factory is None:
        raise RuntimeError(f"Expect model points to be cached for {name} {seed} {num_points} in {dbpath}")

    # the draw runs on the GPU (pvamd_sample_surface): counter-based, so the same (mesh, seed, num_points) gives the same
    # points on any device / launch geometry; open3d's own generator (sdf.py:643-645) cannot be reproduced
    n_init = max(min_init_sample_points, 2 * num_points)
    pts_all, _, keys = obj_factory.sample_surface(n_init, seed)
    keep = torch.argsort(keys)[:num_points]  # sdf.py:650: a random subset, to disperse the samples
    points = pts_all[keep]
    # normals: the face normal at the closest point, from the mesh query itself (sdf.py:652)
    res = obj_factory.object_frame_closest_point(points, compute_normal=True)
    points, normals = points.cpu(), res.normal.cpu()

    cache[name][seed][num_points] = points, normals, None
    if not given_cache and dbpath is not None:
        torch.save(cache, dbpath)
    return points.to(device=device, dtype=dtype), normals.to(device=device, dtype=dtype), cache
