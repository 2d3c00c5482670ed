"""torch.autograd through the cached, composed, robot and grid-chamfer queries.

The reference is plain PyTorch, so its outputs carry an autograd graph wherever its arithmetic is torch ops on the inputs
(sdf.py:399,409,421-426,556-571; model_to_sdf.py:82-115; chamfer.py:82-95).  The Functions here give the same gradient,
given the forward's own decisions (winning leaf, range flag, voxel, active box axes), with HIP kernels for the backward
(csrc/backward.hip).  The callers (CachedSDF.__call__, ComposedSDF.__call__, RobotSDF.set_joint_configuration,
chamfer_partial_sums) route here only when grad mode is on and an input requires grad; otherwise nothing changes.

Double backward is not supported: every backward is once_differentiable, so create_graph=True raises.
"""

import torch
from torch.autograd.function import once_differentiable

from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import transforms as tf

MAX_LEAVES = 64  # pvamd_composed_query_backward: 1 <= S <= 64
# the backward entry point ("cached" / "composed") of each leaf mode; "_f64" is appended for float64
_BACKWARD = {"nearest": "pvamd_{}_query_backward", "trilinear": "pvamd_{}_query_interp_backward"}


def _scratch(S, A, P, f64, dev):
    n = int(_lib.load().pvamd_composed_backward_scratch_bytes(S, A, P, 1 if f64 else 0))
    return _lib.scratch_buffer(max(n, 16), dev)


def _shares_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def _upstream(t, dev, dtype, shape):
    """An incoming gradient as the kernels take it (None stays None: set_materialize_grads(False))."""
    if t is None:
        return None
    return t.detach().reshape(shape).to(device=dev, dtype=dtype).contiguous()


# ---------------------------------------------------------------- CachedSDF.__call__ (sdf.py:535-571)
class CachedQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cached, points):
        ctx.set_materialize_grads(False)
        val, grad = cached(points)  # grad mode is off in here: the usual path, same kernels, same bits
        flat, _, _, _ = _lib.as_query_points(points, cached._packed.device, keep_f64=True)
        if torch.is_tensor(points) and _shares_storage(flat, points):
            # float32 points already contiguous on the device come back as the caller's own storage: an in-place write
            # before backward would move the point the gradient is taken at (the reference's CachedSDF saves nothing and
            # differentiates at the values its forward saw)
            flat = flat.clone()
        ctx.cached, ctx.flat = cached, flat
        ctx.pshape, ctx.pdtype, ctx.pdevice = points.shape, points.dtype, points.device
        # interpolation="trilinear": in range the exact derivative of the interpolated value and gradient w.r.t. the point
        ctx.backward_entry = _BACKWARD[cached.interpolation].format("cached")
        return val, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, dgrad):
        flat, cached = ctx.flat, ctx.cached
        P, dev, dt = flat.shape[0], flat.device, flat.dtype
        dv = _upstream(dval, dev, dt, (P,))
        dg = _upstream(dgrad, dev, dt, (P, 3))
        out = torch.empty((P, 3), dtype=dt, device=dev)
        desc = cached._grid_desc()
        with _lib.on_device(dev):
            _lib.call(ctx.backward_entry, desc, flat, P, dv, dg, out, f64=dt == torch.float64)
        return None, out.reshape(ctx.pshape).to(device=ctx.pdevice, dtype=ctx.pdtype)


def cached_query(cached, points):
    return CachedQuery.apply(cached, points)


# ---------------------------------------------------------------- ComposedSDF.__call__ (sdf.py:392-433)
class ComposedQuery(torch.autograd.Function):
    """Forward: ComposedSDF._fused_forward with out_leaf -- the one dispatch pinned for a grad-requiring call (every dispatch
    gives the same bits; the bucketed one cannot emit leaf ids).  Saved: the points, the detached stack, the leaf id per pair,
    and the inputs themselves for torch's in-place check."""

    @staticmethod
    def forward(ctx, composed, points, tfm, mode):
        ctx.set_materialize_grads(False)
        dev = composed._owner_device()
        val, grad, leaf, flat, tfd = composed._fused_forward(points, mode, want_leaf=True)
        ctx.composed, ctx.flat, ctx.tfd, ctx.leaf, ctx.grids = composed, flat, tfd, leaf, composed._leaf_grids(dev)
        # flat / tfd may alias the inputs (float32 contiguous device tensors are used where they are): saving the inputs lets
        # torch raise on an in-place write between forward and backward, as it does for the reference's matmul (sdf.py:399)
        ctx.save_for_backward(points, tfm)
        ctx.S, ctx.A = len(composed.sdfs), leaf.shape[0]
        ctx.backward_entry = _BACKWARD[mode].format("composed")
        ctx.pshape, ctx.pdtype, ctx.pdevice = points.shape, points.dtype, points.device
        ctx.tdtype, ctx.tdevice = tfm.dtype, tfm.device
        return val, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, dgrad):
        need_p, need_tf = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ctx.saved_tensors  # the version check of the inputs flat / tfd may alias
        flat, tfd, S, A = ctx.flat, ctx.tfd, ctx.S, ctx.A
        P, dev, dt = flat.shape[0], flat.device, flat.dtype
        dv = _upstream(dval, dev, dt, (A, P))
        dg = _upstream(dgrad, dev, dt, (A, P, 3))
        dpoints = torch.empty((P, 3), dtype=dt, device=dev) if need_p else None
        dtf = torch.empty((S * A, 4, 4), dtype=dt, device=dev) if need_tf else None
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            scratch = _scratch(S, A, P, f64, dev)
            _lib.call(ctx.backward_entry, ctx.grids, S, tfd, A, flat, P, ctx.leaf, dv, dg, dpoints, dtf, scratch, f64=f64)
        gp = dpoints.reshape(ctx.pshape).to(device=ctx.pdevice, dtype=ctx.pdtype) if need_p else None
        gt = dtf.to(device=ctx.tdevice, dtype=ctx.tdtype) if need_tf else None
        return None, gp, gt, None


def composed_query(composed, points, mode):
    if len(composed.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(composed.sdfs)}")
    if not torch.is_tensor(points):
        points = torch.as_tensor(points)
    return ComposedQuery.apply(composed, points, composed._tf_matrix, mode)



# ---------------------------------------------------------------- ComposedSDF.min_over_points (include/pvamd.h "Minimum over points")
class MinOverPointsQuery(torch.autograd.Function):
    """Forward: ComposedSDF._min_over_points_fused.  Backward: pvamd_composed_min_over_points_backward over the A (per_leaf: A S)
    selected pairs only -- the gradient of the composed (one-leaf) query gathered at the indices, decisions held fixed."""

    @staticmethod
    def forward(ctx, composed, points, tfm, mode, per_leaf):
        ctx.set_materialize_grads(False)
        dev = composed._owner_device()
        val, idx, grad, idx_k, leaf, flat, tfd = composed._min_over_points_fused(points, mode, per_leaf)
        ctx.mark_non_differentiable(idx)
        ctx.composed, ctx.flat, ctx.tfd, ctx.idx, ctx.leaf, ctx.grids = composed, flat, tfd, idx_k, leaf, composed._leaf_grids(dev)
        ctx.save_for_backward(points, tfm)  # torch's in-place check of the inputs flat / tfd may alias
        ctx.S, ctx.A, ctx.Z = len(composed.sdfs), idx_k.shape[0], idx_k.shape[1]
        ctx.mode, ctx.per_leaf = mode, per_leaf
        ctx.pshape, ctx.pdtype, ctx.pdevice = points.shape, points.dtype, points.device
        ctx.tdtype, ctx.tdevice = tfm.dtype, tfm.device
        return val, idx, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, didx, dgrad):
        need_p, need_tf = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ctx.saved_tensors
        flat, tfd, S, A, Z = ctx.flat, ctx.tfd, ctx.S, ctx.A, ctx.Z
        P, dev, dt = flat.shape[0], flat.device, flat.dtype
        dv = _upstream(dval, dev, dt, (A, Z))
        dg = _upstream(dgrad, dev, dt, (A, Z, 3))
        dpoints = torch.empty((P, 3), dtype=dt, device=dev) if need_p else None
        dtf = torch.empty((S * A, 4, 4), dtype=dt, device=dev) if need_tf else None
        with _lib.on_device(dev):
            scratch = _lib.scratch_buffer(max(_lib.min_over_points_backward_scratch_bytes(S, A, ctx.per_leaf), 16), dev)
            _lib.call("pvamd_composed_min_over_points_backward", ctx.grids, S, tfd, A, flat, P, _lib.LEAF_MODES[ctx.mode],
                      ctx.per_leaf, ctx.idx, ctx.leaf, dv, dg, dpoints, dtf, scratch, f64=dt == torch.float64)
        gp = dpoints.reshape(ctx.pshape).to(device=ctx.pdevice, dtype=ctx.pdtype) if need_p else None
        gt = dtf.to(device=ctx.tdevice, dtype=ctx.tdtype) if need_tf else None
        return None, gp, gt, None, None


def min_over_points(composed, points, mode, per_leaf):
    from pytorch_volumetric_amd.sdf import MinOverPoints
    if len(composed.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(composed.sdfs)}")
    val, idx, grad = MinOverPointsQuery.apply(composed, points, composed._tf_matrix, mode, per_leaf)
    return MinOverPoints(val, idx, grad)

# ---------------------------------------------------------------- ComposedSDF.hinge_over_points (include/pvamd.h "Hinge penalty over points")
class HingeOverPointsQuery(torch.autograd.Function):
    """Forward: ComposedSDF._hinge_over_points_fused.  Backward: pvamd_composed_hinge_over_points_backward over all pairs, the
    composed value and winning leaf recomputed per pair in the kernel -- saved are the flat points and the stack, not the pairs."""

    @staticmethod
    def forward(ctx, composed, points, tfm, margin, power, mode, per_leaf):
        ctx.set_materialize_grads(False)
        dev = composed._owner_device()
        val, cnt, flat, tfd = composed._hinge_over_points_fused(points, margin, power, mode, per_leaf)
        ctx.mark_non_differentiable(cnt)
        ctx.composed, ctx.flat, ctx.tfd, ctx.grids = composed, flat, tfd, composed._leaf_grids(dev)
        ctx.save_for_backward(points, tfm)  # torch's in-place check of the inputs flat / tfd may alias
        ctx.S = len(composed.sdfs)
        ctx.A = tfd.shape[0] // ctx.S
        ctx.margin, ctx.power, ctx.mode, ctx.per_leaf = margin, power, mode, per_leaf
        ctx.pshape, ctx.pdtype, ctx.pdevice = points.shape, points.dtype, points.device
        ctx.tdtype, ctx.tdevice = tfm.dtype, tfm.device
        return val, cnt

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, dcnt):
        need_p, need_tf = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ctx.saved_tensors
        flat, tfd, S, A = ctx.flat, ctx.tfd, ctx.S, ctx.A
        P, dev, dt = flat.shape[0], flat.device, flat.dtype
        Z = S if ctx.per_leaf else 1
        up = _upstream(dval, dev, dt, (A, Z))
        if up is None:  # nothing flows back
            return None, None, None, None, None, None, None
        dpoints = torch.empty((P, 3), dtype=dt, device=dev) if need_p else None
        dtf = torch.empty((S * A, 4, 4), dtype=dt, device=dev) if need_tf else None
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            scratch = _lib.scratch_buffer(max(_lib.hinge_over_points_backward_scratch_bytes(S, A, P, ctx.per_leaf, f64), 16), dev)
            _lib.call("pvamd_composed_hinge_over_points_backward", ctx.grids, S, tfd, A, flat, P, _lib.LEAF_MODES[ctx.mode],
                      ctx.per_leaf, ctx.margin, ctx.power, up, dpoints, dtf, scratch, f64=f64)
        gp = dpoints.reshape(ctx.pshape).to(device=ctx.pdevice, dtype=ctx.pdtype) if need_p else None
        gt = dtf.to(device=ctx.tdevice, dtype=ctx.tdtype) if need_tf else None
        return None, gp, gt, None, None, None, None


def hinge_over_points(composed, points, margin, power, mode, per_leaf):
    from pytorch_volumetric_amd.sdf import HingeOverPoints
    if len(composed.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(composed.sdfs)}")
    val, cnt = HingeOverPointsQuery.apply(composed, points, composed._tf_matrix, margin, power, mode, per_leaf)
    return HingeOverPoints(val, cnt)



# ---------------------------------------------------------------- ComposedSDF.leaf_pair_distance (include/pvamd.h "Leaf-pair distance")
class LeafPairQuery(torch.autograd.Function):
    """Forward: ComposedSDF._leaf_pair_fused.  Backward: pvamd_leaf_pair_distance_backward -- per (configuration, pair) the
    single-pair VJP w.r.t. the pair transform, then the pair transform's VJP to both stack rows, summed per row in pair order."""

    @staticmethod
    def forward(ctx, composed, tfm, plan, mode):
        ctx.set_materialize_grads(False)
        val, idx, grad, idx_k, C, tfd = composed._leaf_pair_fused(plan, mode)
        ctx.mark_non_differentiable(idx)
        ctx.composed, ctx.plan, ctx.mode, ctx.idx, ctx.C, ctx.tfd = composed, plan, mode, idx_k, C, tfd
        ctx.grids = composed._leaf_grids(plan["dev"])
        ctx.save_for_backward(tfm)  # torch's in-place check of the input tfd may alias
        ctx.S, ctx.A, ctx.K = len(composed.sdfs), idx_k.shape[0], idx_k.shape[1]
        ctx.tdtype, ctx.tdevice = tfm.dtype, tfm.device
        return val, idx, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, didx, dgrad):
        ctx.saved_tensors
        plan, S, A, K = ctx.plan, ctx.S, ctx.A, ctx.K
        dev, dt = plan["dev"], plan["dtype"]
        dv = _upstream(dval, dev, dt, (A, K))
        dg = _upstream(dgrad, dev, dt, (A, K, 3))
        dtf = torch.empty((S * A, 4, 4), dtype=dt, device=dev)
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            scratch = _lib.scratch_buffer(_lib.leaf_pair_scratch_bytes(K, A, plan["max_points"], f64, True), dev)
            _lib.call("pvamd_leaf_pair_distance_backward", ctx.grids, S, ctx.tfd, ctx.C, A, plan["packed"], plan["npoints"],
                      plan["table"], K, _lib.LEAF_MODES[ctx.mode], ctx.idx, dv, dg, dtf, scratch, f64=f64)
        return None, dtf.to(device=ctx.tdevice, dtype=ctx.tdtype), None, None


def leaf_pair_distance(composed, plan, mode):
    from pytorch_volumetric_amd.sdf import LeafPairDistance
    if len(composed.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(composed.sdfs)}")
    val, idx, grad = LeafPairQuery.apply(composed, composed._tf_matrix, plan, mode)
    return LeafPairDistance(val, idx, grad)


# ---------------------------------------------------------------- ComposedSDF.leaf_pair_hinge (include/pvamd.h "Leaf-pair hinge")
class LeafPairHingeQuery(torch.autograd.Function):
    """Forward: ComposedSDF._leaf_pair_hinge_fused.  Backward: pvamd_leaf_pair_hinge_backward -- per (configuration, pair) the
    one-leaf hinge's VJP w.r.t. the pair transform, then the pair transform's VJP to both stack rows, summed per row in pair
    order.  The values and decisions are recomputed in the kernel: saved are the plan, the pair transforms and the stack."""

    @staticmethod
    def forward(ctx, composed, tfm, plan, margin, power, mode):
        ctx.set_materialize_grads(False)
        val, cnt, C, tfd = composed._leaf_pair_hinge_fused(plan, margin, power, mode)
        ctx.mark_non_differentiable(cnt)
        ctx.plan, ctx.mode, ctx.C, ctx.tfd, ctx.margin, ctx.power = plan, mode, C, tfd, margin, power
        ctx.grids = composed._leaf_grids(plan["dev"])
        ctx.save_for_backward(tfm)  # torch's in-place check of the input tfd may alias
        ctx.S, ctx.A, ctx.K = len(composed.sdfs), C.shape[1], C.shape[0]
        ctx.tdtype, ctx.tdevice = tfm.dtype, tfm.device
        return val, cnt

    @staticmethod
    @once_differentiable
    def backward(ctx, dval, dcnt):
        ctx.saved_tensors
        plan, S, A, K = ctx.plan, ctx.S, ctx.A, ctx.K
        dev, dt = plan["dev"], plan["dtype"]
        up = _upstream(dval, dev, dt, (A, K))
        if up is None:  # nothing flows back
            return None, None, None, None, None, None
        dtf = torch.empty((S * A, 4, 4), dtype=dt, device=dev)
        f64 = dt == torch.float64
        with _lib.on_device(dev):
            scratch = _lib.scratch_buffer(_lib.leaf_pair_hinge_scratch_bytes(K, A, plan["max_points"], f64, True), dev)
            _lib.call("pvamd_leaf_pair_hinge_backward", ctx.grids, S, ctx.tfd, ctx.C, A, plan["packed"], plan["npoints"],
                      plan["table"], K, plan["max_points"], _lib.LEAF_MODES[ctx.mode], ctx.margin, ctx.power, up, dtf, scratch,
                      f64=f64)
        return None, dtf.to(device=ctx.tdevice, dtype=ctx.tdtype), None, None, None, None


def leaf_pair_hinge(composed, plan, margin, power, mode):
    from pytorch_volumetric_amd.sdf import LeafPairHinge
    if len(composed.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(composed.sdfs)}")
    val, cnt = LeafPairHingeQuery.apply(composed, composed._tf_matrix, plan, margin, power, mode)
    return LeafPairHinge(val, cnt)


# ---------------------------------------------------------------- ray_cast(..., differentiable=True)
# (include/pvamd.h "Ray casting: gradient of the hit distance")
def ray_hit_vjp_torch(d, t, status, n, up):
    """The contract's formula for the rays in float64 torch: directions d (..., 3), the forward's t, status and gradients n, the
    upstream up of t -> (w n, (w t) n), exact zeros where the pair does not contribute.  Not summed over anything."""
    d, t, n, up = (x.to(torch.float64) for x in (d, t, n, up))
    c = n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]
    on = (status == _lib.RAY_HIT) & (c < 0) & torch.isfinite(c)
    w = torch.where(on, -up / torch.where(on, c, torch.ones_like(c)), torch.zeros_like(c))
    zero = torch.zeros_like(n)
    return (torch.where(on.unsqueeze(-1), w.unsqueeze(-1) * n, zero),
            torch.where(on.unsqueeze(-1), (w * t).unsqueeze(-1) * n, zero))


class RayHitDistance(torch.autograd.Function):
    """The generic ray cast's t with its gradient: forward returns the bits of the torch march's t, backward is the contract's
    formula in float64 torch (any SDF, any floating dtype; not a hot path).  origins / directions: the caller's tensors expanded
    to the rays' shape; d, t, status, n: the flat (R, ...) results of the march."""

    @staticmethod
    def forward(ctx, origins, directions, d, t, status, n):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, d, t, status, n)
        return t.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, up):
        origins, directions, d, t, status, n = ctx.saved_tensors
        if up is None:
            return None, None, None, None, None, None
        go, gd = ray_hit_vjp_torch(d, t, status, n, up.detach().to(t.device))
        return (go.reshape(origins.shape).to(device=origins.device, dtype=origins.dtype) if ctx.needs_input_grad[0] else None,
                gd.reshape(directions.shape).to(device=directions.device, dtype=directions.dtype) if ctx.needs_input_grad[1] else None,
                None, None, None, None)


class RayCastQuery(torch.autograd.Function):
    """Forward: the fused ray cast (CachedSDF / ComposedSDF._ray_cast_fused: the usual kernels, the usual bits).  Backward:
    pvamd_cached_ray_cast_backward / pvamd_composed_ray_cast_backward (csrc/ray_cast_backward.hip) from the forward's t, status
    and gradients; a composition recomputes the winning leaf in the kernel.  origins / directions: the caller's tensors expanded
    to the rays' shape (torch's expand backward sums a shared origin); tfm: a composition's stack, else None."""

    @staticmethod
    def forward(ctx, sdf, origins, directions, tfm, o, d, lead, dtype, args):
        ctx.set_materialize_grads(False)
        res, kept = sdf._ray_cast_fused(o, d, lead, dtype, args)
        ctx.kept, ctx.lead = kept, lead
        # the flat rays and the stack the kernels read may alias the inputs, and the results are views of the kernels' buffers:
        # saving them lets torch raise on an in-place write between forward and backward
        ctx.save_for_backward(origins, directions, tfm, kept["out"][0], kept["out"][1], kept["out"][3])
        ctx.mark_non_differentiable(res.status, res.values, res.gradients, res.steps)
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, dt, *_):
        if dt is None:  # nothing flows back
            return (None,) * 9
        origins, directions, tfm = ctx.saved_tensors[:3]  # and the version check of everything saved
        need_o, need_d, need_tf = ctx.needs_input_grad[1:4]
        kept = ctx.kept
        o, d, (t, status, _, grad, _) = kept["o"], kept["d"], kept["out"]
        R, dev, dtype = o.shape[0], o.device, o.dtype
        f64 = dtype == torch.float64
        go = torch.empty((R, 3), dtype=dtype, device=dev) if need_o else None
        gd = torch.empty((R, 3), dtype=dtype, device=dev) if need_d else None
        gtf = None
        if "tfd" not in kept:
            up = _upstream(dt, dev, dtype, (R,))
            with _lib.on_device(dev):
                _lib.call("pvamd_cached_ray_cast_backward", d, R, t, status, grad, up, go, gd, f64=f64)
        else:
            S, A = kept["S"], kept["A"]
            up = _upstream(dt, dev, dtype, (A, R))
            gtf = torch.empty((S * A, 4, 4), dtype=dtype, device=dev) if need_tf else None
            with _lib.on_device(dev):
                scratch = _lib.scratch_buffer(max(_lib.ray_cast_backward_scratch_bytes(S, A, R, f64), 16), dev)
                _lib.call("pvamd_composed_ray_cast_backward", kept["grids"], S, kept["tfd"], A, o, d, R,
                          _lib.LEAF_MODES[kept["mode"]], t, status, up, go, gd, gtf, scratch, f64=f64)
        return (None,
                go.reshape(*ctx.lead, 3).to(device=origins.device, dtype=origins.dtype) if need_o else None,
                gd.reshape(*ctx.lead, 3).to(device=directions.device, dtype=directions.dtype) if need_d else None,
                gtf.to(device=tfm.device, dtype=tfm.dtype) if need_tf else None,
                None, None, None, None, None)


def ray_cast(sdf, graph, o, d, lead, dtype, args):
    """sdf.ray_cast through RayCastQuery: graph = (origins, directions) expanded to the rays' shape, still attached."""
    from pytorch_volumetric_amd.sdf import RayCast
    tfm = getattr(sdf, "_tf_matrix", None)
    if tfm is not None and len(sdf.sdfs) > MAX_LEAVES:
        raise _lib.PvamdError(f"gradients through a composition need at most {MAX_LEAVES} leaves, this one has {len(sdf.sdfs)}")
    return RayCast(*RayCastQuery.apply(sdf, graph[0], graph[1], tfm, o, d, lead, dtype, args))


def pair_transforms_torch(stack, pairs):
    """The pair transforms of include/pvamd.h "Leaf-pair distance" 1 in torch (any dtype, differentiable): stack (S, A, 4, 4),
    pairs (K, 2) -> (K, A, 4, 4).  Rounding aside (torch's matmul does not promise the kernel's fma order), the same C."""
    Ms, Mt = stack[pairs[:, 0]], stack[pairs[:, 1]]
    R = Ms[..., :3, :3] @ Mt[..., :3, :3].transpose(-1, -2)
    t = Ms[..., :3, 3] - (R @ Mt[..., :3, 3:4]).squeeze(-1)
    top = torch.cat((R, t.unsqueeze(-1)), dim=-1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1
    return torch.cat((top, bottom), dim=-2)


class PairTransforms(torch.autograd.Function):
    """Forward: pvamd_leaf_pair_transforms (ComposedSDF._pair_transforms).  Backward (the generic leaf-pair path only): the VJP of
    the same statements in float64 torch on the host, the stack rows summed in pair order -- K x A work, not a hot path."""

    @staticmethod
    def forward(ctx, composed, tfm, table, pairs, dtype, dev):
        ctx.set_materialize_grads(False)
        C, _ = composed._pair_transforms(table, pairs.shape[0], dtype, dev)
        ctx.save_for_backward(tfm)
        ctx.pairs = pairs
        return C

    @staticmethod
    @once_differentiable
    def backward(ctx, dC):
        (tfm,) = ctx.saved_tensors
        if dC is None:
            return None, None, None, None, None, None
        K, A = dC.shape[0], dC.shape[1]
        S = tfm.shape[0] // A
        stack = tfm.detach().to(device="cpu", dtype=torch.float64).reshape(S, A, 4, 4)
        with torch.enable_grad():
            rows = [stack[u].clone().requires_grad_() for u in range(S)]
            C = pair_transforms_torch(torch.stack(rows), ctx.pairs)
            grads = torch.autograd.grad(C, rows, dC.detach().to(device="cpu", dtype=torch.float64), allow_unused=True)
        d = torch.stack([g if g is not None else torch.zeros_like(stack[0]) for g in grads]).reshape(S * A, 4, 4)
        return None, d.to(device=tfm.device, dtype=tfm.dtype), None, None, None, None


def pair_transforms(composed, table, pairs, dtype, dev):
    if composed._tf_grad and torch.is_grad_enabled():
        return PairTransforms.apply(composed, composed._tf_matrix, table, pairs, dtype, dev)
    return composed._pair_transforms(table, pairs.shape[0], dtype, dev)[0]

# ---------------------------------------------------------------- RobotSDF.set_joint_configuration (model_to_sdf.py:82-115)
class ChainConfigure(torch.autograd.Function):
    """Forward: the one-launch HIP configure (pvamd_configure_chain), q (A, M) -> the (S*A, 4, 4) obj->leaf stack.  Backward:
    the VJP of the same statements in float64 torch (forward kinematics, rigid inverse, offset compose) -- A x joints of
    work, not a hot path."""

    @staticmethod
    def forward(ctx, robot, q, configure):
        ctx.set_materialize_grads(False)
        ctx.robot = robot
        ctx.save_for_backward(q)
        return configure(q.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, dstack):
        (q,) = ctx.saved_tensors
        if dstack is None:
            return None, None, None
        with torch.enable_grad():
            q64 = q.detach().to(dtype=torch.float64).requires_grad_()
            stack64 = ctx.robot._stack_torch(q64)
            (dq,) = torch.autograd.grad(stack64, q64, dstack.to(device=stack64.device, dtype=torch.float64))
        return None, dq.to(device=q.device, dtype=q.dtype), None


class TransformStack(torch.autograd.Function):
    """pvamd_transform_stack (stack[s*A+a] = offset_inv[s] @ rigid_inverse(link_world[s*A+a])) for a foreign chain whose
    forward kinematics is torch: the VJP of the same contraction in float64 torch."""

    @staticmethod
    def forward(ctx, offset_inv, link_world, contract):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(offset_inv, link_world)
        return contract(link_world.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, dstack):
        offset_inv, link_world = ctx.saved_tensors
        if dstack is None:
            return None, None, None
        S = offset_inv.shape[0]
        A = link_world.shape[0] // S
        with torch.enable_grad():
            lw = link_world.detach().to(dtype=torch.float64).requires_grad_()
            off = offset_inv.detach().to(device=lw.device, dtype=torch.float64).repeat_interleave(A, dim=0)
            stack64 = off @ tf.rigid_inverse(lw)
            (dlw,) = torch.autograd.grad(stack64, lw, dstack.to(device=lw.device, dtype=torch.float64))
        return None, dlw.to(dtype=link_world.dtype), None


# ---------------------------------------------------------------- batch_chamfer_dist against a cached grid (chamfer.py:82-94)
class GridChamfer(torch.autograd.Function):
    """Per-transform sums of (scale d)^2 over the points (float64), differentiable w.r.t. the world->object matrices and the
    points.  The backward needs nothing beyond the inputs: in-range pairs contribute zero."""

    @staticmethod
    def forward(ctx, cached, W, points, scale):
        ctx.set_materialize_grads(False)
        dev = _lib.require_gpu()
        pts = torch.as_tensor(points).detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        Wd = W.detach().to(device=dev, dtype=torch.float32).contiguous()
        B, N = Wd.shape[0], pts.shape[0]
        sums = torch.empty((B,), dtype=torch.float64, device=dev)
        desc = cached._grid_desc()
        with _lib.on_device(dev):
            _lib.call("pvamd_chamfer_grid", desc, Wd, B, pts, N, float(scale), sums)
        ctx.cached, ctx.Wd, ctx.pts, ctx.scale = cached, Wd, pts, float(scale)
        # Wd / pts may alias W / points: torch's version check then raises on an in-place write before backward, as it does for
        # the reference's matmul (chamfer.py:82)
        ctx.save_for_backward(W, points if torch.is_tensor(points) else None)
        ctx.wdtype, ctx.wdevice = W.dtype, W.device
        ctx.pshape, ctx.pdtype, ctx.pdevice = points.shape, points.dtype, points.device
        return sums

    @staticmethod
    @once_differentiable
    def backward(ctx, dsums):
        need_w, need_p = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if dsums is None:
            return None, None, None, None
        ctx.saved_tensors  # the version check of the inputs Wd / pts may alias
        Wd, pts = ctx.Wd, ctx.pts
        B, N, dev = Wd.shape[0], pts.shape[0], pts.device
        dsum = dsums.detach().reshape(B).to(device=dev, dtype=torch.float32).contiguous()
        dW = torch.empty((B, 4, 4), dtype=torch.float32, device=dev) if need_w else None
        dp = torch.empty((N, 3), dtype=torch.float32, device=dev) if need_p else None
        desc = ctx.cached._grid_desc()
        with _lib.on_device(dev):
            scratch = _scratch(1, B, N, False, dev)
            _lib.call("pvamd_chamfer_grid_backward", desc, Wd, B, pts, N, ctx.scale, dsum, dW, dp, scratch)
        gw = dW.to(device=ctx.wdevice, dtype=ctx.wdtype) if need_w else None
        gp = dp.reshape(ctx.pshape).to(device=ctx.pdevice, dtype=ctx.pdtype) if need_p else None
        return None, gw, gp, None


def grid_chamfer_sums(cached, W, points, scale):
    return GridChamfer.apply(cached, W, points, scale)
