"""RobotSDF: an SDF of an articulated robot, conditioned on (batched) joint configurations
(reference model_to_sdf.py:12-133).  One leaf per mesh visual; forward kinematics gives world_T_link per
configuration; `pvamd_transform_stack` (f32 MFMA) contracts them with the visual offsets into the leaf-major
object->leaf stack that the fused ComposedSDF kernel consumes."""
import ctypes
import logging
import math
import typing

import numpy as np
import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import sdf
from pytorch_volumetric_amd import transforms as tf

logger = logging.getLogger(__file__)


class RobotSDF(sdf.ObjectFrameSDF):
    """SDF for a robot model described by a kinematic chain (pytorch_volumetric_amd.kinematics.Chain or a
    pytorch_kinematics.Chain); the joint configuration must be set before querying."""

    def __init__(self, chain, default_joint_config=None, path_prefix='',
                 link_sdf_cls: typing.Callable[[sdf.ObjectFactory], sdf.ObjectFrameSDF] = sdf.MeshSDF):
        """
        :param chain: robot description; links with non-mesh visuals are ignored (with a warning)
        :param default_joint_config: joint values used until set_joint_configuration is called; None = zeros
        :param path_prefix: prefix for the relative mesh paths found in the robot description
        :param link_sdf_cls: factory of each link's SDF from its ObjectFactory (MeshSDF, or cache_link_sdf_factory())
        """
        self.chain = chain
        self.dtype = self.chain.dtype
        self.device = self.chain.device
        self.q = None
        self._stack, self._stack_obj = None, None  # object_to_link_frames: the (S*A, 4, 4) stack / the Transform3d around it
        self.joint_names = self.chain.get_joint_parameter_names()
        self.frame_names = self.chain.get_frame_names(exclude_fixed=False)
        self.sdf: typing.Optional[sdf.ComposedSDF] = None
        self.sdf_to_link_name = []
        self.link_factories = []
        self.configuration_batch = None
        self._sc_points, self._sc_pairs = None, None  # set_self_collision_points / self_collision_pairs

        sdfs, offsets = self._collect_mesh_links(path_prefix, link_sdf_cls)
        self.offset_transforms = tf.Transform3d(matrix=torch.cat([tf.as_matrix(o) for o in offsets], dim=0)).to(
            device=self.device, dtype=self.dtype)
        self.sdf = sdf.ComposedSDF(sdfs, self.object_to_link_frames)
        self.set_joint_configuration(default_joint_config)

    def _collect_mesh_links(self, path_prefix, link_sdf_cls):
        """One leaf SDF (+ its visual offset) per mesh visual of the chain, in frame order (model_to_sdf.py:41-56)."""
        sdfs, offsets = [], []
        for link in (self.chain.find_frame(name).link for name in self.frame_names):
            for visual in link.visuals:
                if visual.geom_type != "mesh":
                    logger.warning(f"Cannot handle non-mesh link visual type {visual} for {link.name}")
                    continue
                mesh_file, mesh_scale = visual.geom_param[0], visual.geom_param[1]
                factory = sdf.MeshObjectFactory(mesh_file, scale=mesh_scale, path_prefix=path_prefix)
                sdfs.append(link_sdf_cls(factory))
                self.link_factories.append(factory)  # each leaf's mesh, for set_self_collision_points
                offsets.append(visual.offset)
                self.sdf_to_link_name.append(link.name)
        if not sdfs:
            raise RuntimeError("robot description has no mesh visuals to build an SDF from")
        return sdfs, offsets

    def surface_bounding_box(self, **kwargs):
        return self.sdf.surface_bounding_box(**kwargs)

    def link_bounding_boxes(self):
        """[A x] S x 8 x 3 corner points of each link's bounding box in the robot frame under the current
        configuration (model_to_sdf.py:65-80)."""
        tfs = tf.Transform3d(matrix=tf.rigid_inverse(tf.as_matrix(self.sdf.obj_frame_to_link_frame)))
        bbs = []
        for i in range(len(self.sdf.sdfs)):
            bb = aabb_to_ordered_end_points(np.asarray(self.sdf.sdfs[i].surface_bounding_box(padding=0)))
            bb = torch.tensor(bb, device=tfs.device, dtype=tfs.dtype)
            bbs.append(tfs[self.sdf.ith_transform_slice(i)].transform_points(bb))
        return torch.stack(bbs).squeeze()

    def set_joint_configuration(self, joint_config=None):
        """
        :param joint_config: [A x] M joint values; A may be any number of batch dimensions (model_to_sdf.py:82-115)
        """
        M = len(self.joint_names)
        if joint_config is None:
            joint_config = torch.zeros(M, device=self.device, dtype=self.dtype)
        joint_config = torch.as_tensor(joint_config)
        if joint_config.dim() == 0 or joint_config.shape[-1] != M:
            # (the kernel reads q[a * M + joint]: a short float32 GPU vector, used where it is, would be read out of bounds)
            raise ValueError(f"joint configuration of shape {tuple(joint_config.shape)} does not hold the {M} joint values "
                             f"({', '.join(self.joint_names)}) in its last dimension")
        if len(joint_config.shape) > 1:
            self.configuration_batch = tuple(joint_config.shape[:-1])
            # a chain of fixed joints only has M == 0: reshape(-1, 0) cannot infer the batch
            joint_config = joint_config.reshape(math.prod(self.configuration_batch), M)
        else:
            self.configuration_batch = None
        self.q = joint_config
        S = len(self.sdf_to_link_name)
        lib = _lib.load()
        dev = _lib.require_gpu()
        offset_inv = self._offset_inv_dev(dev)
        # gradients to q (autograd.py): the same launches inside a Function whose backward is the VJP of the same statements
        want_grad = joint_config.requires_grad and torch.is_grad_enabled()
        with _lib.on_device(dev):
            if hasattr(self.chain, "joint_table"):
                # ONE launch (pvamd_configure_chain): sin / cos + frame walk + offset^-1 o world^-1 on the f32 MFMA.  Joint values
                # that already sit on this GPU as float32 (A, M) are used where they are; anything else is one H2D copy.
                A = 1 if joint_config.dim() == 1 else joint_config.shape[0]

                def configure(jc):
                    if jc.is_cuda and jc.dtype is torch.float32 and jc.device == dev and jc.is_contiguous():
                        q = jc
                    else:
                        q = jc.reshape(A, M).to(device=dev, dtype=torch.float32).contiguous()
                    return self._configure(lib, dev, q, A, M, S, offset_inv)

                if want_grad:
                    from pytorch_volumetric_amd import autograd
                    stack = autograd.ChainConfigure.apply(self, joint_config.reshape(A, M), configure)
                else:
                    stack = configure(joint_config)
            else:
                # a foreign chain object (e.g. pytorch_kinematics.Chain): use its own forward kinematics
                fk = self.chain.forward_kinematics(joint_config, end_only=False)
                link_world = torch.cat([tf.as_matrix(fk[name]) for name in self.sdf_to_link_name])  # leaf-major
                A = link_world.shape[0] // S
                link_world_d = link_world.to(device=dev, dtype=torch.float32).contiguous()

                def contract(lw):
                    # object_to_link[s*A+a] = offset[s]^-1 @ world_T_link[s,a]^-1 on the matrix cores
                    out = torch.empty_like(lw)
                    _lib.call("pvamd_transform_stack", offset_inv, lw, S, A, out)
                    return out

                if link_world_d.requires_grad and torch.is_grad_enabled():
                    from pytorch_volumetric_amd import autograd
                    stack = autograd.TransformStack.apply(offset_inv, link_world_d, contract)
                else:
                    stack = contract(link_world_d)
        self._stack, self._stack_obj = stack, None  # the Transform3d is built when object_to_link_frames is read
        if self.sdf is not None:
            self.sdf.set_transforms(stack, batch_dim=self.configuration_batch, known_rigid=True)

    @property
    def object_to_link_frames(self) -> typing.Optional[tf.Transform3d]:
        """model_to_sdf.py:113: the [A*]S object -> link transforms of the current configuration, leaf-major."""
        if self._stack_obj is None and self._stack is not None:
            # configure_and_query_into re-writes its stack in place on the next call: what the caller holds must not change
            # under it (the reference returns a fresh object per configuration)
            own = any(hit[1] is self._stack for hit in self.__dict__.get("_cfg_stack", {}).values())
            self._stack_obj = tf.Transform3d(matrix=self._stack.clone() if own else self._stack)
        return self._stack_obj

    @object_to_link_frames.setter
    def object_to_link_frames(self, value):
        self._stack_obj = value
        self._stack = None if value is None else tf.as_matrix(value)

    def _configure(self, lib, dev, q, A, M, S, offset_inv, stack=None, sincos=None, one_launch_only=False):
        """pvamd_configure_chain on the current stream: q (A, M) float32 on `dev` -> the (S*A, 4, 4) obj->leaf stack.  The
        frame scratch is kept per (device, stream, batch size): it is private to one call on one stream, and two streams that
        configure the same robot concurrently must not share it.  A robot with more SDF-carrying links than the one-launch
        kernel can stage in LDS (PVAMD_E_SHAPE, ~50 links) takes sin / cos + pvamd_chain_fk + pvamd_transform_stack -- the same
        fma chains, any S -- unless the caller needs the single launch (`one_launch_only`: graph capture)."""
        joints, F = self._joint_table_dev(dev)
        stream = _lib.stream_ptr()
        key = (str(dev), stream.value, A)
        hit = self._per_stream("_cfg_scratch", key, lambda: torch.empty((F, 12, A), dtype=torch.float32, device=dev))
        if stack is None:
            stack = torch.empty((S * A, 4, 4), dtype=torch.float32, device=dev)
        rc = lib.pvamd_configure_chain(joints.data_ptr(), F, q.data_ptr(), A, M, offset_inv.data_ptr(), S,
                                       None if sincos is None else sincos.data_ptr(), hit[1].data_ptr(), None,
                                       stack.data_ptr(), stream)
        if rc == _lib.E_SHAPE and not one_launch_only:  # (a shape the three-launch path rejects as well is reported there)
            sin_q, cos_q = torch.sin(q), torch.cos(q)
            if sincos is not None:
                sincos.copy_(torch.stack((sin_q, cos_q), dim=-1))
            link_world = torch.empty((S * A, 4, 4), dtype=torch.float32, device=dev)
            _lib.check(lib.pvamd_chain_fk(joints.data_ptr(), F, q.data_ptr(), sin_q.data_ptr(), cos_q.data_ptr(), A, M,
                                          hit[1].data_ptr(), link_world.data_ptr(), stream), "pvamd_chain_fk")
            _lib.check(lib.pvamd_transform_stack(offset_inv.data_ptr(), link_world.data_ptr(), S, A, stack.data_ptr(), stream),
                       "pvamd_transform_stack")
        elif rc == _lib.E_SHAPE and one_launch_only:
            lds = S * 12 * 64 * 4 + F * ctypes.sizeof(_lib.JointDesc) + 64 * M * 2 * 4
            raise ValueError(f"configure_and_query_into: pvamd_configure_chain refused the shape (frames F={F}, joints M={M}, "
                             f"SDF-carrying links S={S}, configurations A={A}); the one-launch configure kernel needs F, A, S >= 1 and "
                             f"{lds} bytes of LDS (limit 153600: about 50 SDF-carrying links); otherwise call "
                             "set_joint_configuration(q) and query_into(...) instead")
        elif rc != 0:
            _lib.check(rc, "pvamd_configure_chain")
        return stack

    def _per_stream(self, name, key, make):
        """(key, tensor) of a buffer kept per (device, stream, batch size); at most 8 keys are remembered."""
        table = self.__dict__.setdefault(name, {})
        hit = table.get(key)
        if hit is None:
            if len(table) >= 8:
                table.pop(next(iter(table)))
            hit = table[key] = (key, make())
        return hit

    def configure_and_query_into(self, joint_config, points, out_val, out_grad):
        """A planner's inner step without host work between its two launches: joint values (A, M) float32 ALREADY ON THE GPU
        -> pvamd_configure_chain -> pvamd_composed_query into the caller's (A, P) / (A, P, 3) buffers (for large batches on small
        link grids the query is the chunk-grouped pair, ComposedSDF.group_points: one more launch).  No host data, no
        allocation after the first call with this batch size: capturable in a hipGraph (model_to_sdf.py:82-125 as two
        or three kernels).  Needs a kinematics.Chain (on-device FK) and BOUNDING_BOX CachedSDF leaves; afterwards the object is
        configured exactly as by set_joint_configuration(joint_config)."""
        sdf._require_nearest(self.sdf, "configure_and_query_into")
        if not hasattr(self.chain, "joint_table"):
            raise ValueError("configure_and_query_into needs the on-device forward kinematics (pytorch_volumetric_amd.kinematics.Chain)")
        M, S = len(self.joint_names), len(self.sdf_to_link_name)
        q = joint_config
        if not (torch.is_tensor(q) and q.is_cuda and q.dtype is torch.float32 and q.dim() == 2 and q.shape[1] == M and q.is_contiguous()):
            raise ValueError(f"configure_and_query_into needs contiguous float32 (A, {M}) joint values on the GPU")
        A = q.shape[0]
        dev = q.device
        lib = _lib.load()
        with _lib.on_device(dev):
            key = (str(dev), _lib.current_raw_stream(dev.index), A)
            # the stack this entry point writes is its own (per stream), re-used call after call
            hit = self._per_stream("_cfg_stack", key, lambda: torch.empty((S * A, 4, 4), dtype=torch.float32, device=dev))
            self._configure(lib, dev, q, A, M, S, self._offset_inv_dev(dev), stack=hit[1], one_launch_only=True)
            self.q, self.configuration_batch = q, (A,)
            if self._stack is not hit[1]:
                self._stack = hit[1]
            self._stack_obj = None  # a Transform3d handed out earlier keeps the configuration it was read under (a copy)
            cur = self.sdf._tf_matrix
            if cur is None or cur.data_ptr() != hit[1].data_ptr() or cur.shape != hit[1].shape or self.sdf.tsf_batch != (A,):
                self.sdf.set_transforms(hit[1], batch_dim=(A,), known_rigid=True)
            self.sdf.invalidate_transforms()  # this stack is re-written in place: drop everything derived from its old contents
            self.sdf.query_into(points, out_val, out_grad)

    def _stack_torch(self, q):
        """The (S*A, 4, 4) obj->leaf stack of joint values q (A, M) in torch, in q's dtype on q's device: forward kinematics,
        rigid inverse, offset compose (model_to_sdf.py:94-113) -- what ChainConfigure differentiates (autograd.py)."""
        key = (q.dtype, str(q.device))
        cached = self.__dict__.get("_chain_torch")
        if cached is None or cached[0] != key:
            cached = self._chain_torch = (key, self.chain.to(dtype=q.dtype, device=q.device))
        fk = cached[1].forward_kinematics(q, end_only=False)
        link_world = torch.cat([tf.as_matrix(fk[name]) for name in self.sdf_to_link_name])  # leaf-major
        A = q.shape[0]
        off = tf.rigid_inverse(self.offset_transforms.get_matrix().to(device=q.device, dtype=q.dtype))
        return off.repeat_interleave(A, dim=0) @ tf.rigid_inverse(link_world)

    def _offset_inv_dev(self, dev):
        if getattr(self, "_offset_inv_cache", None) is None or self._offset_inv_cache.device != dev:
            self._offset_inv_cache = tf.rigid_inverse(self.offset_transforms.get_matrix()).to(
                device=dev, dtype=torch.float32).contiguous()
        return self._offset_inv_cache

    def _joint_table_dev(self, dev):
        if getattr(self, "_joint_cache", None) is None or self._joint_cache[0].device != dev:
            raw = self.chain.joint_table(self.sdf_to_link_name)
            t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
            import ctypes
            self._joint_cache = (t, len(raw) // ctypes.sizeof(_lib.JointDesc))
        return self._joint_cache

    def __call__(self, points_in_object_frame):
        """
        :param points_in_object_frame: [B x] N x 3 points in the robot frame
        :return: [A x] [B x] N values and [A x] [B x] N x 3 gradients (A = configuration batch dims)
        """
        return self.sdf(points_in_object_frame)

    def min_over_points(self, points, per_leaf=False):
        """ComposedSDF.min_over_points under the current joint configuration: per configuration (and per link with per_leaf;
        leaf s is sdf_to_link_name[s]) the closest point of `points`, its value and gradient.  Differentiable w.r.t. q when
        set_joint_configuration was given a q that requires grad, as __call__ is."""
        return self.sdf.min_over_points(points, per_leaf=per_leaf)

    def hinge_over_points(self, points, margin, power=2, per_leaf=False):
        """ComposedSDF.hinge_over_points under the current joint configuration: per configuration (and per link with per_leaf;
        leaf s is sdf_to_link_name[s]) the clearance cost sum_p max(margin - v, 0) ** power and the count of points inside the
        margin.  Differentiable w.r.t. q when set_joint_configuration was given a q that requires grad, as __call__ is."""
        return self.sdf.hinge_over_points(points, margin, power=power, per_leaf=per_leaf)

    def ray_cast(self, origins, directions, t_min=0., t_max=math.inf, hit_tolerance=1e-3, step_scale=1., max_steps=128,
                 differentiable=False):
        """ComposedSDF.ray_cast under the current joint configuration: per configuration and ray (rays in the robot frame, shared
        by the configurations) where the ray first meets the robot -- a depth or lidar sensor simulated against every
        configuration at once.  The result carries no autograd graph unless differentiable=True: then t is differentiable
        w.r.t. the rays and, when set_joint_configuration was given a q that requires grad, w.r.t. q (the surface-normal
        linearisation at the hit point; include/pvamd.h "Ray casting: gradient of the hit distance")."""
        return self.sdf.ray_cast(origins, directions, t_min=t_min, t_max=t_max, hit_tolerance=hit_tolerance,
                                 step_scale=step_scale, max_steps=max_steps, differentiable=differentiable)

    def set_self_collision_points(self, points=None, num_points=256, seed=0):
        """The point set of each leaf that self_collision_distance moves against the other leaves' SDFs.

        :param points: None: num_points surface samples per leaf from that leaf's own mesh (sample_mesh_points, seed `seed`, no
            cache file); else a sequence of S tensors (P_s, 3), each in its leaf's frame (leaf s is sdf_to_link_name[s])
        The points are packed onto the GPU once, with the pair table of the default pairs."""
        S = len(self.sdf_to_link_name)
        if points is None:
            dev = _lib.require_gpu()
            points = [sdf.sample_mesh_points(f, num_points=num_points, seed=seed, dbpath=None, device=dev)[0]
                      for f in self.link_factories]
        elif isinstance(points, torch.Tensor) or len(points) != S:
            raise ValueError(f"points must be a sequence of {S} point sets, one per leaf")
        pts = []
        for i, p in enumerate(points):
            p = torch.as_tensor(p)
            if p.dim() != 2 or p.shape[-1] != 3:
                raise ValueError(f"points[{i}] must have shape (P, 3), got {tuple(p.shape)}")
            pts.append(p.detach().to(dtype=p.dtype if p.dtype == torch.float64 else torch.float32).contiguous())
        self._sc_points = pts
        if self.sdf._tf_matrix is not None and self.self_collision_pairs().shape[0]:
            self.sdf._leaf_pair_plan(self._sc_points, self.self_collision_pairs())

    def self_collision_pairs(self):
        """The default (K, 2) int64 table of ordered leaf pairs for self_collision_distance: every ordered pair of non-adjacent
        leaves (model_to_sdf.self_collision_pairs), sorted by (s, t)."""
        if self._sc_pairs is None:
            self._sc_pairs = self_collision_pairs(self.chain, self.sdf_to_link_name)
        return self._sc_pairs

    def self_collision_distance(self, pairs=None):
        """ComposedSDF.leaf_pair_distance of the self-collision points (set_self_collision_points; sampled with its defaults on
        first use) under the current joint configuration.  Per configuration and pair (s, t): how close leaf t's points come to
        leaf s -- values, indices into leaf t's points, and gradients in leaf t's frame.  The two directions of a pair are
        different queries; torch.minimum of the two gives the symmetric distance.  Differentiable w.r.t. q when
        set_joint_configuration was given a q that requires grad.

        :param pairs: int (K, 2) ordered leaf pairs; None = self_collision_pairs()
        :return: LeafPairDistance(values, indices, gradients) of shapes [A] + (K,), [A] + (K,), [A] + (K, 3)"""
        if self._sc_points is None:
            self.set_self_collision_points()
        return self.sdf.leaf_pair_distance(self._sc_points, self.self_collision_pairs() if pairs is None else pairs)

    def self_collision_hinge(self, margin, power=2, pairs=None):
        """ComposedSDF.leaf_pair_hinge of the self-collision points (set_self_collision_points; sampled with its defaults on
        first use) under the current joint configuration: per configuration and pair (s, t), the sum over leaf t's points of
        max(margin - v, 0) ** power under leaf s's SDF, and the count of points with v < margin -- the self-collision half of a
        CHOMP, TrajOpt or MPPI cost (values.sum(-1) sums it over the pairs).  Differentiable w.r.t. q when
        set_joint_configuration was given a q that requires grad.  With nearest link grids only points outside a link's grid
        range move q; trilinear link grids (cache_link_sdf_factory(..., interpolation="trilinear")) give a gradient everywhere.

        :param margin: a finite Python real number; :param power: 1 or 2
        :param pairs: int (K, 2) ordered leaf pairs; None = self_collision_pairs()
        :return: LeafPairHinge(values, counts), both of shape [A] + (K,)"""
        if self._sc_points is None:
            self.set_self_collision_points()
        return self.sdf.leaf_pair_hinge(self._sc_points, self.self_collision_pairs() if pairs is None else pairs, margin,
                                        power=power)

    def link_pair_transforms(self, pairs=None):
        """ComposedSDF.leaf_pair_transforms under the current joint configuration: [A] + (K, 4, 4) leaf t frame -> leaf s frame
        transforms of the pairs (None = self_collision_pairs())."""
        return self.sdf.leaf_pair_transforms(self.self_collision_pairs() if pairs is None else pairs)

    def query_into(self, points, out_val, out_grad):
        """Allocation-free form of __call__ (see ComposedSDF.query_into); outputs are (A,P) and (A,P,3)."""
        self.sdf.query_into(points, out_val, out_grad)

    def prepare_points(self, points_in_object_frame):
        """Sort a re-used query point set once (ComposedSDF.prepare_points); query it under every later joint configuration
        with query_prepared(handle, order="caller" | "sorted")."""
        return self.sdf.prepare_points(points_in_object_frame)

    def query_prepared(self, prepared, order="caller"):
        return self.sdf.query_prepared(prepared, order=order)


def _link_parents(chain):
    """{link name: parent link name or None} of a kinematic tree: a kinematics.Chain's frames, or a pytorch_kinematics chain's
    frame tree (its root frame and the children of each frame)."""
    frames = getattr(chain, "_frames", None)
    if frames is not None and all(hasattr(f, "parent") and hasattr(f, "link") for f in frames):
        return {f.link.name: (None if f.parent is None else frames[f.parent].link.name) for f in frames}
    root = getattr(chain, "_root", None)
    if root is not None and hasattr(root, "children") and hasattr(root, "link"):
        parents, todo = {root.link.name: None}, [root]
        while todo:
            f = todo.pop()
            for c in f.children:
                parents[c.link.name] = f.link.name
                todo.append(c)
        return parents
    raise ValueError("cannot read the kinematic tree of this chain to choose the self-collision pairs; pass pairs explicitly")


def self_collision_pairs(chain, sdf_to_link_name):
    """The default self-collision pairs of a robot (host only): every ordered pair (s, t), s != t, of non-adjacent leaves, sorted
    by (s, t), as an int64 (K, 2) tensor.  Leaves are adjacent when they belong to the same link, or when one leaf's link is the
    nearest leaf-carrying ancestor of the other's (links without a leaf are collapsed, so a mesh-less link between two meshed
    links does not hide their joint).  Both directions are listed, because they are different queries (the points of t
    against the SDF of s); torch.minimum of the two gives the symmetric distance.

    :param chain: a kinematics.Chain or a pytorch_kinematics chain (its frame tree); anything else raises ValueError
    :param sdf_to_link_name: the link of each leaf (RobotSDF.sdf_to_link_name)"""
    parents = _link_parents(chain)
    names = list(sdf_to_link_name)
    missing = sorted(set(names) - set(parents))
    if missing:
        raise ValueError(f"links {missing} are not in the chain's kinematic tree; pass pairs explicitly")
    meshed = set(names)

    def carrier(name):  # the nearest leaf-carrying ancestor
        p = parents[name]
        while p is not None and p not in meshed:
            p = parents.get(p)
        return p

    anc = {n: carrier(n) for n in meshed}
    out = [(s, t) for s in range(len(names)) for t in range(len(names))
           if s != t and names[s] != names[t] and anc[names[s]] != names[t] and anc[names[t]] != names[s]]
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2)


def cache_link_sdf_factory(resolution=0.01, padding=0.1, **kwargs):
    """model_to_sdf.py:128-133"""

    def create_sdf(obj_factory: sdf.ObjectFactory):
        gt_sdf = sdf.MeshSDF(obj_factory)
        return sdf.CachedSDF(obj_factory.name, resolution, obj_factory.bounding_box(padding=padding), gt_sdf, **kwargs)

    return create_sdf


_CORNER_ORDER = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1))
_SEQUENTIAL_ORDER = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0),
                     (1, 0, 1), (1, 1, 1), (1, 1, 0), (1, 1, 1), (0, 1, 1), (0, 1, 0), (0, 1, 1), (0, 0, 1))


def aabb_to_ordered_end_points(aabb, arrange_in_sequential_order=False):
    """8 corners (or the 16-vertex wireframe polyline) of a (3,2) [[min,max],...] box, in the reference's order
    (model_to_sdf.py:136-171)."""
    order = _SEQUENTIAL_ORDER if arrange_in_sequential_order else _CORNER_ORDER
    arr = [[aabb[d, pick[d]] for d in range(3)] for pick in order]
    if torch.is_tensor(aabb):
        return torch.tensor(arr, device=aabb.device, dtype=aabb.dtype)
    return np.array(arr)
