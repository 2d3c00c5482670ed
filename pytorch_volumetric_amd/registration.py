"""Second-order pose refinement against an SDF: the Gauss-Newton normal equations of the chamfer cost
sum_i (scale * sdf(W p_i))^2 over a left-multiplied twist of every pose (`chamfer_normal_equations`, one fused pass over the
(pose, point) pairs) and a Levenberg-Marquardt loop around them whose decisions stay on the device (`refine_poses`).
`semantic_normal_equations` is the same pass with a kind (surface, free, occupied, ignore) and a target distance per point and
Huber weights; `refine_poses` runs on it when asked for any of the three.
The contracts are include/pvamd.h "Chamfer normal equations" and "Semantic normal equations"; the kernels are
csrc/registration.hip."""
import math
import numbers
from typing import NamedTuple

import torch

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import transforms as tf
from pytorch_volumetric_amd.sdf import CachedSDF, ObjectFrameSDF, OutOfBoundsStrategy

LAMBDA_MIN = 1e-12
LAMBDA_MAX = 1e12
POINT_SURFACE = _lib.POINT_SURFACE    # penalised on either side of its target distance
POINT_FREE = _lib.POINT_FREE          # penalised only where the object reaches it: sdf < target
POINT_OCCUPIED = _lib.POINT_OCCUPIED  # penalised only where the object does not: sdf > target
POINT_IGNORE = _lib.POINT_IGNORE      # never penalised, like every value outside 0..3


class ChamferNormalEquations(NamedTuple):
    cost: torch.Tensor      # (B,) float64: scale^2 / N * sum v^2, what batch_chamfer_dist returns before its cast
    gradient: torch.Tensor  # (B, 6) float64: scale^2 / N * sum v j, half of d cost / d xi at xi = 0; xi = (u, w)
    hessian: torch.Tensor   # (B, 6, 6) float64: scale^2 / N * sum j j^T, symmetric
    counts: torch.Tensor    # (B,) int64: points of the pose inside the grid range


class SemanticNormalEquations(NamedTuple):
    cost: torch.Tensor      # (B,) float64: scale^2 / N * sum rho(r), rho the Huber function (r^2 inside huber_delta)
    gradient: torch.Tensor  # (B, 6) float64: scale^2 / N * sum w r j over the active pairs
    hessian: torch.Tensor   # (B, 6, 6) float64: scale^2 / N * sum w j j^T over the active pairs, symmetric
    counts: torch.Tensor    # (B,) int64: points of the pose inside the grid range, whatever their kind
    active: torch.Tensor    # (B, 3) int64: active pairs of kind POINT_SURFACE, POINT_FREE, POINT_OCCUPIED
    outliers: torch.Tensor  # (B,) int64: active pairs with |r| > huber_delta


class PoseRefinement(NamedTuple):
    world_to_object: torch.Tensor  # (B, 4, 4) the best accepted pose, in the input's dtype and device
    cost: torch.Tensor             # (B,) float64 its cost
    initial_cost: torch.Tensor     # (B,) float64 the cost of the input pose
    accepted: torch.Tensor         # (B,) int64 evaluations accepted (the first one included)


def _check_scale(scale):
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
        raise TypeError(f"scale must be a real number, got {scale!r}")
    if not math.isfinite(scale):
        raise ValueError(f"scale must be finite, got {scale!r}")
    return float(scale)


def _check_points(points):
    pts = points if torch.is_tensor(points) else torch.as_tensor(points)
    if pts.dim() < 1 or pts.shape[-1] != 3:
        raise ValueError(f"points must have last dimension 3, got {tuple(pts.shape)}")
    if pts.numel() == 0:
        raise ValueError("points must hold at least one point (the cost is a mean over them)")
    return pts


def _check_inputs(world_to_object, points, obj_sdf):
    """(W (B, 4, 4) as given, points as a tensor); raises before anything touches the device."""
    if not isinstance(obj_sdf, ObjectFrameSDF):
        raise TypeError(f"obj_sdf must be an ObjectFrameSDF, got {type(obj_sdf).__name__}")
    W = tf.as_matrix(world_to_object)
    if W.dim() != 3 or tuple(W.shape[1:]) != (4, 4):
        raise ValueError(f"world_to_object must be (B, 4, 4), got {tuple(W.shape)}")
    return W, _check_points(points)


def _fused_mode(obj_sdf):
    """The leaf mode of the fused kernel, or None for the generic path."""
    if isinstance(obj_sdf, CachedSDF) and obj_sdf._dim == 3 and \
            obj_sdf.out_of_bounds_strategy == OutOfBoundsStrategy.BOUNDING_BOX and obj_sdf.interpolation in _lib.LEAF_MODES:
        return _lib.LEAF_MODES[obj_sdf.interpolation]
    return None


def _device_of(obj_sdf, mode):
    return obj_sdf._packed.device if mode is not None else _lib.require_gpu()


_TRIANGLE = {}


def _triangle_index(dev, M):
    """(M * M,) index into the packed upper triangle, cached per (device, M) (creating it copies from the host)."""
    idx = _TRIANGLE.get((dev, M))
    if idx is None:
        rows, e = [[0] * M for _ in range(M)], 0
        for r in range(M):
            for c in range(r, M):
                rows[r][c] = rows[c][r] = e
                e += 1
        idx = _TRIANGLE[(dev, M)] = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(-1)
    return idx


def _check_semantic_args(pts, semantics, targets, huber_delta):
    """(semantics, targets as tensors where given, huber_delta as a float or None); raises before anything touches the device."""
    lead = tuple(pts.shape[:-1])

    def per_point(name, val, what, floating_ok):
        if val is None:
            return None
        if not torch.is_tensor(val):
            try:
                val = torch.as_tensor(val)
            except (TypeError, ValueError, RuntimeError) as e:
                raise TypeError(f"{name} must be {what} tensor, got {type(val).__name__}") from e
        if val.dtype == torch.bool or val.dtype.is_complex or (val.dtype.is_floating_point and not floating_ok):
            raise TypeError(f"{name} must have {what} dtype, got {val.dtype}")
        if tuple(val.shape) != lead:
            raise ValueError(f"{name} must have the shape of points without its last dimension {lead}, got {tuple(val.shape)}")
        return val

    semantics = per_point("semantics", semantics, "an integer", False)
    targets = per_point("targets", targets, "a real", True)
    if huber_delta is not None:
        if isinstance(huber_delta, bool) or not isinstance(huber_delta, numbers.Real):
            raise TypeError(f"huber_delta must be a real number, got {huber_delta!r}")
        if not huber_delta > 0:  # a NaN too; inf switches the weights off
            raise ValueError(f"huber_delta must be positive, got {huber_delta!r}")
        huber_delta = float(huber_delta)
    return semantics, targets, huber_delta


def _prepare_semantics(semantics, targets, dev):
    """(kinds (N,) uint8, targets (N,) float32) on the device, None where not given.  A kind outside 0..3 means POINT_IGNORE:
    mapped on the device, before the narrowing cast could fold it into range, without a synchronisation."""
    kinds = None
    if semantics is not None:
        s = semantics.detach().reshape(-1).to(device=dev)
        kinds = torch.where((s >= POINT_SURFACE) & (s <= POINT_IGNORE), s, POINT_IGNORE).to(torch.uint8).contiguous()
    if targets is not None:
        targets = targets.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    return kinds, targets


class _Evaluator:
    """The raw sums (B, 28) and counts at float32 poses (B, 4, 4) on the device; buffers allocated once.  plain: "Chamfer normal
    equations", counts (B,).  Otherwise "Semantic normal equations", the five counts (B, 5): kinds (N,) uint8 and targets (N,)
    float32 on the device, or None; delta a float (inf: plain least squares)."""

    def __init__(self, obj_sdf, mode, dev, pts, B, kinds=None, targets=None, delta=math.inf, plain=False):
        self.obj_sdf, self.mode, self.dev, self.pts, self.B = obj_sdf, mode, dev, pts, B
        self.kinds, self.targets, self.delta, self.plain = kinds, targets, delta, plain
        self.N = pts.shape[0]
        self.sums = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device=dev)
        self.counts = torch.empty((B,) if plain else (B, _lib.SEM_COUNTS), dtype=torch.int64, device=dev)
        if mode is not None:
            size = _lib.chamfer_normal_eq_scratch_bytes if plain else _lib.semantic_normal_eq_scratch_bytes
            self.scratch = torch.empty((size(B, self.N) // 8,), dtype=torch.int64, device=dev)
            self.desc = obj_sdf._grid_desc()

    def __call__(self, W32):
        if self.B == 0:
            return
        if self.mode is not None:
            head = (self.desc, self.mode, W32, self.B, self.pts, self.N)
            tail = (self.sums, self.counts, self.scratch)
            if self.plain:
                _lib.call("pvamd_chamfer_normal_eq", *head, *tail)
            else:
                _lib.call("pvamd_semantic_normal_eq", *head, self.kinds, self.targets, self.delta, *tail)
            return
        # any other object: transform with the kernel's statements, query the object, the contract's statements in float64 in torch.
        # One block serves the plain form too: without kinds and targets and with delta = inf every pair is active and none an
        # outlier, and a `where` on an all-true mask, a product with 1.0 and `a > inf` change no bit of v v, v j and j j^T
        x = torch.empty((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
        _lib.call("pvamd_transform_points", W32, self.B, self.pts, self.N, x)
        with torch.no_grad():
            v, n = self.obj_sdf(x)
        v = v.detach().to(device=self.dev, dtype=torch.float64).reshape(self.B, self.N)
        n = n.detach().to(device=self.dev, dtype=torch.float64).reshape(self.B, self.N, 3)
        j = torch.cat((n, torch.linalg.cross(x.to(torch.float64), n, dim=-1)), dim=-1)
        r = v if self.targets is None else v - self.targets.to(torch.float64)
        if self.kinds is None:
            surface = torch.ones_like(r, dtype=torch.bool)
            free = occupied = torch.zeros_like(surface)
        else:
            surface = (self.kinds == POINT_SURFACE).expand(self.B, self.N)
            free = (self.kinds == POINT_FREE) & ~(r >= 0)
            occupied = (self.kinds == POINT_OCCUPIED) & ~(r <= 0)
        active = surface | free | occupied
        a = r.abs()
        outlier = active & (a > self.delta)
        w = torch.where(outlier, self.delta / a, 1.0)  # times one is exact: an inlier enters as (r, j)
        zero = torch.zeros((), dtype=torch.float64, device=self.dev)
        # inactive pairs are left out by selection, not by a product with zero: their NaN stays out of the sums
        self.sums[:, 0] = torch.where(active, torch.where(outlier, self.delta * ((a + a) - self.delta), r * r), zero).sum(-1)
        self.sums[:, 1:7] = torch.where(active.unsqueeze(-1), (w * r).unsqueeze(-1) * j, zero).sum(-2)
        rr, cc = torch.triu_indices(6, 6).tolist()
        self.sums[:, 7:] = torch.where(active.unsqueeze(-1), (w.unsqueeze(-1) * j)[..., rr] * j[..., cc], zero).sum(-2)
        if self.plain:
            self.counts.fill_(self.N)  # no grid: every point is answered by the object itself
            return
        self.counts[:, 0] = self.N
        self.counts[:, 1] = (active & surface).sum(-1)
        self.counts[:, 2] = free.sum(-1)
        self.counts[:, 3] = occupied.sum(-1)
        self.counts[:, 4] = outlier.sum(-1)


def _prepare(W, pts, dev):
    pts32 = pts.detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
    W32 = W.detach().to(device=dev, dtype=torch.float32).contiguous()
    return W32, pts32


def chamfer_normal_equations(world_to_object, points, obj_sdf: ObjectFrameSDF, scale=1000.):
    """The Gauss-Newton normal equations of `batch_chamfer_dist(world_to_object, points, obj_sdf=obj_sdf, scale=scale)` over a
    left-multiplied twist xi = (u, w) of every pose, translation first: x' = x + w x x + u.

    :param world_to_object: (B, 4, 4) transforms (or a transform object), used in float32 as batch_chamfer_dist uses them
    :param points: (N, 3) world-frame points, N >= 1 (leading dimensions are flattened)
    :param obj_sdf: the object; a 3-D BOUNDING_BOX CachedSDF (nearest or trilinear) runs one fused kernel, anything else
        is transformed, queried and summed in torch under the same contract
    :param scale: unit conversion applied to the distance before squaring
    :return: ChamferNormalEquations(cost (B,), gradient (B, 6), hessian (B, 6, 6), counts (B,)) on the GPU, float64 / int64.
        Per pair, v and n are the value and the gradient the object returns at x = W p, j = (n, x cross n) in float64;
        cost = scale^2 / N sum v^2, gradient = scale^2 / N sum v j, hessian = scale^2 / N sum j j^T.  The sums are float64 in
        an order that depends only on (B, N): two calls give the same bits.  A NaN makes its own pose's outputs NaN.  The
        result carries no autograd graph (it is a solver's input).  No device -> host synchronisation: the call can be
        captured in a graph once the object's descriptor exists (after one call)."""
    scale = _check_scale(scale)
    W, pts = _check_inputs(world_to_object, points, obj_sdf)
    mode = _fused_mode(obj_sdf)
    dev = _device_of(obj_sdf, mode)
    with _lib.on_device(dev):
        W32, pts32 = _prepare(W, pts, dev)
        ev = _Evaluator(obj_sdf, mode, dev, pts32, W32.shape[0], plain=True)
        ev(W32)
        k = scale * scale / ev.N
        s = ev.sums * k
        return ChamferNormalEquations(s[:, 0], s[:, 1:7], s[:, 7:][:, _triangle_index(dev, 6)].reshape(-1, 6, 6), ev.counts)


def semantic_normal_equations(world_to_object, points, obj_sdf: ObjectFrameSDF, scale=1000., semantics=None, targets=None,
                              huber_delta=None):
    """`chamfer_normal_equations` for points that are not all surface points, with Huber weights: the normal equations of
    scale^2 / N sum_i rho(r_i), r = sdf(W p_i) - target_i, over the pairs that are active under their point's kind.

    :param semantics: integer tensor of shape points.shape[:-1], the kind of every point: POINT_SURFACE (0) is penalised on
        either side, POINT_FREE (1) only where r < 0 (the object reaches into known free space), POINT_OCCUPIED (2) only where
        r > 0, POINT_IGNORE (3) and every value outside 0..3 never.  None: every point is a surface point
    :param targets: real tensor of the same shape, the distance each point should have (float32 on the device).  None: 0
    :param huber_delta: a positive number in the units of the SDF (before scale): a pair with |r| > huber_delta enters with the
        weight w = huber_delta / |r| and the cost huber_delta (2 |r| - huber_delta).  None or inf: w = 1
    :return: SemanticNormalEquations(cost (B,), gradient (B, 6), hessian (B, 6, 6), counts (B,), active (B, 3), outliers (B,)) on
        the GPU, float64 / int64: cost = scale^2 / N sum rho, gradient = scale^2 / N sum w r j, hessian = scale^2 / N sum w j j^T
        with j as in chamfer_normal_equations and N every point, ignored ones included.  An inactive pair adds nothing, whatever
        the object returns there.  With all three options None the first four fields are chamfer_normal_equations' bit for bit
        (from another kernel: include/pvamd.h "Semantic normal equations").  Same order, same reproducibility, no autograd
        graph, no device -> host synchronisation."""
    scale = _check_scale(scale)
    W, pts = _check_inputs(world_to_object, points, obj_sdf)
    semantics, targets, huber_delta = _check_semantic_args(pts, semantics, targets, huber_delta)
    mode = _fused_mode(obj_sdf)
    dev = _device_of(obj_sdf, mode)
    with _lib.on_device(dev):
        W32, pts32 = _prepare(W, pts, dev)
        kinds, targets32 = _prepare_semantics(semantics, targets, dev)
        ev = _Evaluator(obj_sdf, mode, dev, pts32, W32.shape[0], kinds, targets32, math.inf if huber_delta is None else huber_delta)
        ev(W32)
        k = scale * scale / ev.N
        s = ev.sums * k
        return SemanticNormalEquations(s[:, 0], s[:, 1:7], s[:, 7:][:, _triangle_index(dev, 6)].reshape(-1, 6, 6), ev.counts[:, 0],
                                       ev.counts[:, 1:4], ev.counts[:, 4])


def _check_refine_args(iterations, damping, damping_up, damping_down):
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral):
        raise TypeError(f"iterations must be an int, got {iterations!r}")
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations}")
    for name, val in (("damping", damping), ("damping_up", damping_up), ("damping_down", damping_down)):
        if isinstance(val, bool) or not isinstance(val, numbers.Real):
            raise TypeError(f"{name} must be a real number, got {val!r}")
    if not (math.isfinite(damping) and damping > 0):
        raise ValueError(f"damping must be finite and positive, got {damping!r}")
    if not (math.isfinite(damping_up) and damping_up > 1):
        raise ValueError(f"damping_up must be finite and above 1, got {damping_up!r}")
    if not (0 < damping_down <= 1):
        raise ValueError(f"damping_down must lie in (0, 1], got {damping_down!r}")
    return int(iterations), float(damping), float(damping_up), float(damping_down)


def refine_poses(world_to_object, points, obj_sdf: ObjectFrameSDF, iterations=10, scale=1000., damping=1e-3, damping_up=10.,
                 damping_down=0.1, semantics=None, targets=None, huber_delta=None):
    """Levenberg-Marquardt refinement of B poses against an SDF: minimises the chamfer cost of `chamfer_normal_equations` by
    damped Gauss-Newton steps, every accept / reject decision taken on the device (pvamd_pose_lm_step).  With any of semantics,
    targets and huber_delta given it minimises the cost of `semantic_normal_equations` (their meaning is stated there) by the
    same loop and step; with all three None it runs the kernels and gives the bits it always did.

    :param iterations: normal-equation evaluations after the initial one, an int >= 1
    :param damping: initial Marquardt damping (relative to the Hessian's diagonal), multiplied by damping_down after an
        accepted evaluation and by damping_up after a rejected one, kept within [LAMBDA_MIN, LAMBDA_MAX]
    :return: PoseRefinement(world_to_object, cost, initial_cost, accepted): the best accepted pose of every input pose (never
        worse than the input: cost <= initial_cost) in the input's dtype and device, its cost and the input's (float64), and
        the number of accepted evaluations (>= 1: the first).  A fixed sequence of 1 + iterations x (normal equations, step)
        launches with no device -> host synchronisation: the call can be captured in a graph."""
    scale = _check_scale(scale)
    iterations, damping, up, down = _check_refine_args(iterations, damping, damping_up, damping_down)
    W, pts = _check_inputs(world_to_object, points, obj_sdf)
    plain = semantics is None and targets is None and huber_delta is None
    semantics, targets, huber_delta = _check_semantic_args(pts, semantics, targets, huber_delta)
    out_dtype = W.dtype if W.dtype.is_floating_point else torch.float32
    out_device = W.device
    mode = _fused_mode(obj_sdf)
    dev = _device_of(obj_sdf, mode)
    with _lib.on_device(dev):
        W32, pts32 = _prepare(W, pts, dev)
        B = W32.shape[0]
        kinds, targets32 = _prepare_semantics(semantics, targets, dev)
        ev = _Evaluator(obj_sdf, mode, dev, pts32, B, kinds, targets32, math.inf if huber_delta is None else huber_delta, plain)
        # the state of pvamd_pose_lm_step
        w_try = W32[:, :3, :].to(torch.float64).contiguous()
        w_acc = torch.empty_like(w_try)
        sums_acc = torch.empty_like(ev.sums)
        lam = torch.full((B,), damping, dtype=torch.float64, device=dev)
        accepted = torch.zeros((B,), dtype=torch.int32, device=dev)
        w_next = W32.clone()
        initial = None
        for it in range(iterations + 1):
            ev(w_next)
            if it == 0:
                initial = ev.sums[:, 0].clone()
            _lib.call("pvamd_pose_lm_step", B, ev.sums, it == 0, w_acc, sums_acc, lam, accepted, w_try, w_next, up, down,
                      LAMBDA_MIN, LAMBDA_MAX)
        k = scale * scale / ev.N
        out = torch.zeros((B, 4, 4), dtype=out_dtype, device=dev)
        out[:, :3, :] = w_acc.to(out_dtype)
        out[:, 3, 3] = 1
        return PoseRefinement(out.to(out_device), sums_acc[:, 0] * k, initial * k, accepted.to(torch.int64))
