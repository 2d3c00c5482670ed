"""Second-order refinement of a robot's joint values against a point cloud: the articulated sibling of registration.py.
`joint_normal_equations` gives the Gauss-Newton normal equations of the cost of `semantic_normal_equations`, taken over the joint
values of a RobotSDF instead of a rigid pose, in one fused pass over the (configuration, point) pairs;
`refine_joint_configuration` is the Levenberg-Marquardt loop around them whose decisions stay on the device.

Every point is won by exactly one leaf and a link's twist Jacobian J_s does not depend on the point, so the joint-space equations
factor exactly over the leaves: H = sum_s J_s^T H6_s J_s, g = sum_s J_s^T g6_s, with (c_s, g6_s, H6_s) the 28 sums of the
semantic normal equations over the points leaf s wins.  The per-point work is the composed walk and those 28 fused multiply-adds,
whatever the number of joints.  The contract is include/pvamd.h "Joint-space normal equations"; the kernels are
csrc/articulated.hip."""
import math
from typing import NamedTuple

import numpy as np
import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import kinematics
from pytorch_volumetric_amd import registration as reg
from pytorch_volumetric_amd.model_to_sdf import RobotSDF
from pytorch_volumetric_amd.sdf import CachedSDF, OutOfBoundsStrategy


class JointNormalEquations(NamedTuple):
    cost: torch.Tensor         # (A,) float64: scale^2 / N * sum rho(r) over the active pairs
    gradient: torch.Tensor     # (A, M) float64: scale^2 / N * sum w r J^T j, half of d cost / d q under the linearisation
    hessian: torch.Tensor      # (A, M, M) float64: scale^2 / N * sum w J^T j j^T J, exactly symmetric
    counts: torch.Tensor       # (A,) int64: points inside the grid range of the leaf that wins them
    active: torch.Tensor       # (A, 3) int64: active pairs of kind POINT_SURFACE, POINT_FREE, POINT_OCCUPIED
    outliers: torch.Tensor     # (A,) int64: active pairs with |r| > huber_delta
    leaf_active: torch.Tensor  # (A, S) int64: active pairs every leaf won -- which links the cloud observes


class JointRefinement(NamedTuple):
    joint_config: torch.Tensor  # (A, M) the best accepted joint values, in the input's dtype and device
    cost: torch.Tensor          # (A,) float64 their cost
    initial_cost: torch.Tensor  # (A,) float64 the cost of the input
    accepted: torch.Tensor      # (A,) int64 evaluations accepted (the first one included)


def _check_robot(robot):
    """(S, M, leaf mode) of a robot the fused kernels serve; anything else raises, naming the condition.  Host only."""
    if not isinstance(robot, RobotSDF):
        raise TypeError(f"robot must be a RobotSDF, got {type(robot).__name__}")
    if not isinstance(robot.chain, kinematics.Chain):
        raise ValueError(f"joint refinement needs the on-device forward kinematics of pytorch_volumetric_amd.kinematics.Chain; the "
                         f"robot's chain is a {type(robot.chain).__name__}")
    leaves = list(robot.sdf.sdfs)
    for s, leaf in enumerate(leaves):
        if not (isinstance(leaf, CachedSDF) and leaf._dim == 3 and leaf.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX
                and leaf.interpolation in _lib.LEAF_MODES):
            raise ValueError(f"joint refinement needs every link to be a 3-D BOUNDING_BOX CachedSDF (cache_link_sdf_factory); leaf "
                             f"{s} ({robot.sdf_to_link_name[s]}) is a {type(leaf).__name__}")
    modes = sorted({leaf.interpolation for leaf in leaves})
    if len(modes) != 1:
        raise ValueError(f"joint refinement needs one interpolation for every link, got {modes}")
    S, M = len(leaves), len(robot.joint_names)
    if S > _lib.JOINT_MAX_LEAVES:
        raise ValueError(f"joint refinement serves at most {_lib.JOINT_MAX_LEAVES} leaves, the robot has {S}")
    if M > _lib.JOINT_MAX:
        raise ValueError(f"joint refinement serves at most {_lib.JOINT_MAX} joints, the robot has {M}")
    return S, M, _lib.LEAF_MODES[modes[0]]


def _check_config(joint_config, M, names):
    """joint_config as an (A, M) tensor (not yet on the device)."""
    q = joint_config if torch.is_tensor(joint_config) else torch.as_tensor(joint_config)
    if q.dtype == torch.bool or q.dtype.is_complex:
        raise TypeError(f"joint_config must have a real dtype, got {q.dtype}")
    if q.dim() not in (1, 2) or q.shape[-1] != M:
        raise ValueError(f"joint_config must be ({M},) or (A, {M}): the values of {', '.join(names) if names else 'no joints'}; got "
                         f"{tuple(q.shape)}")
    return q.reshape(1, M) if q.dim() == 1 else q


def _check_limits(joint_limits, M):
    """joint_limits as an (M, 2) float64 array whose bounds are float32 values inside the caller's, or None.  The step clamps in
    float64 and the result is rounded to float32: bounds that are float32 values keep the rounded result inside them."""
    if joint_limits is None:
        return None
    lim = joint_limits if torch.is_tensor(joint_limits) else torch.as_tensor(joint_limits)
    if lim.dtype == torch.bool or lim.dtype.is_complex:
        raise TypeError(f"joint_limits must have a real dtype, got {lim.dtype}")
    if tuple(lim.shape) != (M, 2):
        raise ValueError(f"joint_limits must be ({M}, 2): (lower, upper) of every joint; got {tuple(lim.shape)}")
    lim = lim.detach().to(device="cpu", dtype=torch.float64).numpy()
    if not (lim[:, 0] <= lim[:, 1]).all():  # a NaN too
        raise ValueError("joint_limits must have lower <= upper for every joint (and no NaN)")
    lo, hi = lim[:, 0].astype(np.float32), lim[:, 1].astype(np.float32)
    lo = np.where(lo.astype(np.float64) < lim[:, 0], np.nextafter(lo, np.float32(np.inf)), lo).astype(np.float64)
    hi = np.where(hi.astype(np.float64) > lim[:, 1], np.nextafter(hi, np.float32(-np.inf)), hi).astype(np.float64)
    if not (lo <= hi).all():
        raise ValueError("joint_limits leave no float32 value between the lower and the upper bound of some joint")
    return np.stack((lo, hi), axis=-1)


class _Evaluator:
    """The raw sums (A, 1 + M + M (M + 1) / 2) and counts (A, 5 + S) at float32 joint values (A, M) on the device; every buffer,
    the stack included, is this object's own: the robot stays configured as it was."""

    def __init__(self, robot, S, M, mode, dev, pts, A, kinds, targets, delta):
        self.robot, self.S, self.M, self.mode, self.dev, self.pts, self.A = robot, S, M, mode, dev, pts, A
        self.kinds, self.targets, self.delta = kinds, targets, delta
        self.N = pts.shape[0]
        self.P = 1 + M + M * (M + 1) // 2
        self.grids = robot.sdf._leaf_grids(dev)
        self.joints, self.F = robot._joint_table_dev(dev)
        self.offset_inv = robot._offset_inv_dev(dev)
        f64, i64 = torch.float64, torch.int64
        self.stack = torch.empty((S * A, 4, 4), dtype=torch.float32, device=dev)
        self.leaf_sums = torch.empty((A, S, _lib.REG_SUMS), dtype=f64, device=dev)
        self.leaf_counts = torch.empty((A, S, _lib.SEM_COUNTS), dtype=i64, device=dev)
        self.J = torch.empty((A, S, 6, M), dtype=f64, device=dev)
        self.sums = torch.empty((A, self.P), dtype=f64, device=dev)
        self.counts = torch.empty((A, _lib.SEM_COUNTS + S), dtype=i64, device=dev)
        self.scratch = _lib.scratch_buffer(_lib.joint_normal_eq_scratch_bytes(A, S, self.N), dev)

    def __call__(self, q32):
        if self.A == 0:
            return
        self.robot._configure(_lib.load(), self.dev, q32, self.A, self.M, self.S, self.offset_inv, stack=self.stack)
        _lib.call("pvamd_joint_normal_eq", self.grids, self.S, self.mode, self.stack, self.A, self.pts, self.N, self.kinds,
                  self.targets, self.delta, self.leaf_sums, self.leaf_counts, self.scratch)
        _lib.call("pvamd_chain_twists", self.joints, self.F, q32, self.A, self.M, self.offset_inv, self.S, self.J)
        _lib.call("pvamd_joint_assemble", self.leaf_sums, self.leaf_counts, self.J, self.A, self.S, self.M, self.sums, self.counts)


def _prepare(robot, joint_config, points, semantics, targets, huber_delta):
    """The argument checks of both entry points, all on the host: (S, M, mode, q (A, M), points, semantics, targets, delta)."""
    S, M, mode = _check_robot(robot)
    q = _check_config(joint_config, M, robot.joint_names)
    pts = reg._check_points(points)
    semantics, targets, huber_delta = reg._check_semantic_args(pts, semantics, targets, huber_delta)
    return S, M, mode, q, pts, semantics, targets, math.inf if huber_delta is None else huber_delta


def _evaluator(robot, dev, S, M, mode, q, pts, semantics, targets, delta):
    q32, pts32 = reg._prepare(q, pts, dev)
    kinds, targets32 = reg._prepare_semantics(semantics, targets, dev)
    return _Evaluator(robot, S, M, mode, dev, pts32, q32.shape[0], kinds, targets32, delta), q32


def joint_normal_equations(robot: RobotSDF, joint_config, points, scale=1000., semantics=None, targets=None, huber_delta=None):
    """The Gauss-Newton normal equations of scale^2 / N sum_i rho(robot_sdf(p_i; q) - target_i) over the joint values q: what
    `semantic_normal_equations` is for a rigid pose, for a robot.

    :param robot: a RobotSDF on a kinematics.Chain whose links are all 3-D BOUNDING_BOX CachedSDFs of one interpolation
        (cache_link_sdf_factory), with at most 64 leaves and 32 joints; anything else raises ValueError naming the condition.
        Its current configuration is left as it is
    :param joint_config: (M,) or (A, M) joint values, used in float32 as set_joint_configuration uses them
    :param points: (..., 3) points in the robot's object frame (what robot(points) takes), N >= 1 after flattening
    :param scale, semantics, targets, huber_delta: as in semantic_normal_equations
    :return: JointNormalEquations on the GPU, float64 / int64.  Per (configuration, point) the winning leaf, the leaf-frame point x
        and the leaf's own (v, n) are those of robot(points); r, the activity, the Huber weight and j = (n, x cross n) are those of
        semantic_normal_equations; with J the 6 x M twist Jacobian of the winning leaf, cost = scale^2 / N sum rho,
        gradient = scale^2 / N sum w r J^T j, hessian = scale^2 / N sum w J^T j j^T J (exactly symmetric).  The sums are float64 in
        a fixed order: two calls give the same bits.  A NaN makes its own configuration's outputs NaN.  No autograd graph, no
        device -> host synchronisation: the call can be captured in a graph after one call."""
    scale = reg._check_scale(scale)
    S, M, mode, q, pts, semantics, targets, delta = _prepare(robot, joint_config, points, semantics, targets, huber_delta)
    dev = robot.sdf._owner_device()
    with _lib.on_device(dev):
        ev, q32 = _evaluator(robot, dev, S, M, mode, q, pts, semantics, targets, delta)
        ev(q32)
        s = ev.sums * (scale * scale / ev.N)
        C = _lib.SEM_COUNTS
        return JointNormalEquations(s[:, 0], s[:, 1:1 + M], s[:, 1 + M:][:, reg._triangle_index(dev, M)].reshape(ev.A, M, M),
                                    ev.counts[:, 0], ev.counts[:, 1:4], ev.counts[:, 4], ev.counts[:, C:])


def refine_joint_configuration(robot: RobotSDF, joint_config, points, iterations=10, scale=1000., damping=1e-3, damping_up=10.,
                               damping_down=0.1, semantics=None, targets=None, huber_delta=None, joint_limits=None):
    """Levenberg-Marquardt refinement of A joint configurations of a robot against a point cloud: minimises the cost of
    `joint_normal_equations` by damped Gauss-Newton steps, every accept / reject decision taken on the device
    (pvamd_joint_lm_step) -- `refine_poses` in joint space.

    :param iterations, damping, damping_up, damping_down: as in refine_poses
    :param joint_limits: None, or a real (M, 2) tensor of (lower, upper) per joint, lower <= upper (read on the host).  Every
        step is clamped into them, and so is joint_config before its first evaluation: no returned value lies outside
    :return: JointRefinement(joint_config (A, M), cost, initial_cost, accepted): the best accepted joint values of every input
        configuration (cost <= initial_cost always) in the input's dtype and device, their cost and the input's (float64), and the
        number of accepted evaluations (>= 1: the first).  A fixed sequence of 1 + iterations x (configure, normal equations,
        twists, assembly, step) launches with nothing read back.  A robot without joints (M = 0) is evaluated once and the input
        returned."""
    scale = reg._check_scale(scale)
    iterations, damping, up, down = reg._check_refine_args(iterations, damping, damping_up, damping_down)
    S, M, mode, q, pts, semantics, targets, delta = _prepare(robot, joint_config, points, semantics, targets, huber_delta)
    limits = _check_limits(joint_limits, M)
    out_dtype = q.dtype if q.dtype.is_floating_point else torch.float32
    out_device = q.device
    dev = robot.sdf._owner_device()
    with _lib.on_device(dev):
        ev, q32 = _evaluator(robot, dev, S, M, mode, q, pts, semantics, targets, delta)
        A = ev.A
        lim = None
        if limits is not None and M > 0:
            lim = torch.from_numpy(limits).to(dev)
            q32 = torch.minimum(torch.maximum(q32, lim[:, 0].to(torch.float32)), lim[:, 1].to(torch.float32))
        # the state of pvamd_joint_lm_step
        q_try = q32.to(torch.float64).contiguous()
        q_acc = q_try.clone()  # (what M = 0 and A = 0 return)
        sums_acc = torch.empty_like(ev.sums)
        lam = torch.full((A,), damping, dtype=torch.float64, device=dev)
        accepted = torch.zeros((A,), dtype=torch.int32, device=dev)
        q_next = q32.clone()
        initial = torch.empty((A,), dtype=torch.float64, device=dev)
        for it in range((iterations if M > 0 else 0) + 1):
            ev(q_next)
            if it == 0:
                initial = ev.sums[:, 0].clone()
            _lib.call("pvamd_joint_lm_step", A, M, ev.sums, it == 0, q_acc, sums_acc, lam, accepted, q_try, q_next, lim,
                      up, down, reg.LAMBDA_MIN, reg.LAMBDA_MAX)
        k = scale * scale / ev.N
        return JointRefinement(q_acc.to(out_dtype).to(out_device), sums_acc[:, 0] * k, initial * k, accepted.to(torch.int64))
