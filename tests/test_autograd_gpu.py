"""-m gpu: gradients through torch autograd (pytorch_volumetric_amd/autograd.py, csrc/backward.hip) against the reference's
expressions run with autograd in float64 (oracle.torch_opforop), given the forward's decisions."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from oracle.torch_opforop import CachedOpForOp, ComposedOpForOp
from pytorch_volumetric_amd import transforms as tf
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-4  # pairs whose decisions could flip within this distance of a boundary are dropped (gradcheck eps is 1e-6)


@pytest.fixture(scope="module")
def cached():
    return W.build_c2_cache()


@pytest.fixture(scope="module")
def robot():
    return W.build_c4()


def ref_leaf(c, device="cpu"):
    """float64 CachedOpForOp over the same grid."""
    packed = c._packed.double().to(device)
    v = c._view
    return CachedOpForOp(packed[:, 0].reshape(v.shape).contiguous(), packed[:, 1:4].contiguous(),
                         v.min.double().to(device), v.max.double().to(device), c.bb.double().to(device))


def stable(c, x):
    """(...,) bool: x (leaf frame, float64) is at least TOL away from every boundary that decides the forward: the range, the
    surface box faces, and (in range) the half-voxel planes of its index."""
    v = c._view
    vmin, vmax = v.min.double().to(x.device), v.max.double().to(x.device)
    bb = c.bb.double().to(x.device)
    res = (vmax - vmin) / (torch.tensor(v.shape, device=x.device, dtype=torch.float64) - 1)
    ok = ((x - vmin).abs() > TOL).all(-1) & ((x - vmax).abs() > TOL).all(-1)
    ok &= ((x - bb[:, 0]).abs() > TOL).all(-1) & ((x - bb[:, 1]).abs() > TOL).all(-1)
    inside = ((vmin <= x) & (x <= vmax)).all(-1)
    q = (x - vmin) / res
    half = ((q - torch.floor(q) - 0.5).abs() * res > TOL).all(-1)
    return ok & (~inside | half)


def composed_decisions(leaves, m64, pts64, A):
    """Restatement of the composed forward per leaf: (A, P) winner, and a mask of pairs whose winner is decided by more than
    TOL (value margin to the runner-up) and whose leaf-frame point is stable()."""
    S = len(leaves)
    x = pts64.unsqueeze(0) @ m64[:, :3, :3].transpose(-1, -2) + m64[:, None, :3, 3]
    x = x.reshape(S, A, -1, 3)
    vals = torch.stack([ref_leaf(c, pts64.device)(x[s])[0] for s, c in enumerate(leaves)])  # (S, A, P)
    best = vals.argmin(0)
    srt = vals.sort(0).values
    margin = (srt[1] - srt[0]) if S > 1 else torch.full_like(srt[0], math.inf)
    st = torch.stack([stable(c, x[s]) for s, c in enumerate(leaves)])
    ok = (margin > TOL) & st.gather(0, best.unsqueeze(0)).squeeze(0)
    return best, ok


def pose_matrices(params):
    """(n, 6) translation + axis-angle -> (n, 4, 4) rigid, differentiable (Rodrigues in torch)."""
    t, w = params[:, :3], params[:, 3:]
    th = w.norm(dim=-1, keepdim=True)
    k = w / th
    K = torch.zeros(params.shape[0], 3, 3, dtype=params.dtype, device=params.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    eye = torch.eye(3, dtype=params.dtype, device=params.device).expand_as(K)
    s, c = torch.sin(th)[..., None], torch.cos(th)[..., None]
    R = eye + s * K + (1 - c) * (K @ K)
    top = torch.cat((R, t.unsqueeze(-1)), dim=-1)
    bottom = torch.tensor([0, 0, 0, 1], dtype=params.dtype, device=params.device).expand(params.shape[0], 1, 4)
    return torch.cat((top, bottom), dim=1)


def cached_points(c, n, seed):
    """Points in range and outside on one, two and three axes, away from every decision boundary."""
    pts = W.c2_points(c, n, seed, margin=0.3).double()
    return pts[stable(c, pts)].contiguous()


# ---------------------------------------------------------------- cached
@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
def test_cached_gradient_matches_torch_restatement(cached, upstream):
    pts = cached_points(cached, 20000, seed=3)
    lo, hi = cached.bb[:, 0].double().cpu(), cached.bb[:, 1].double().cpu()
    v = cached._view
    inside = ((v.min.double() <= pts.cpu()) & (pts.cpu() <= v.max.double())).all(-1)
    out_axes = ((pts.cpu() < lo) | (pts.cpu() > hi)).sum(-1)
    for k in (1, 2, 3):
        assert int((~inside & (out_axes == k)).sum()) >= 100, f"too few points outside on {k} axes"
    assert int(inside.sum()) >= 500
    g = torch.Generator().manual_seed(5)
    wv = torch.randn(pts.shape[0], generator=g, dtype=torch.float64)
    wg = torch.randn(pts.shape[0], 3, generator=g, dtype=torch.float64)

    def loss(val, grad):
        out = 0
        if upstream in ("val", "both"):
            out = out + (val.double() * wv.to(val.device)).sum()
        if upstream in ("grad", "both"):
            out = out + (grad.double() * wg.to(grad.device)).sum()
        return out

    p32 = pts.float().cuda().requires_grad_()
    val, grad = cached(p32)
    assert val.grad_fn is not None and grad.grad_fn is not None
    loss(val, grad).backward()
    p64 = pts.float().double().cpu().requires_grad_()
    rv, rg = ref_leaf(cached)(p64)
    loss(rv, rg).backward()
    got, want = p32.grad.double().cpu(), p64.grad
    assert torch.equal(got[inside], torch.zeros_like(got[inside]))
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())


def test_cached_gradcheck_float64(cached):
    pts = cached_points(cached, 2000, seed=7)[:200].cuda().requires_grad_()
    assert pts.shape[0] >= 150
    assert torch.autograd.gradcheck(lambda p: cached(p), (pts,), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)


def test_cached_gradient_independent_of_size_dispatch(cached):
    """The cached forward dispatches on P (scalar / direct / wave-tile kernels); the backward gives the same bits per point."""
    base = W.c2_points(cached, 40000, seed=11)
    grads = []
    for n in (1000, 20000, 40000):
        p = base[:n].clone().requires_grad_()
        v, g = cached(p)
        (v.sum() + g.sum()).backward()
        grads.append(p.grad[:1000].clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


# ---------------------------------------------------------------- composed
def test_composed_gradcheck_points_and_pose_float64(cached):
    S, A = 3, 4
    comp = pv.ComposedSDF([cached] * S, None)
    params = torch.cat((torch.randn(S * A, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.05,
                        torch.randn(S * A, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)), dim=1).cuda()
    pts = H.uniform_points(600, [-0.3] * 3, [0.3] * 3, seed=4).double().cuda()
    with torch.no_grad():
        _, ok = composed_decisions([cached] * S, pose_matrices(params), pts, A)
    keep = ok.all(0)  # points whose decisions are stable under every configuration
    pts = pts[keep].contiguous()
    assert pts.shape[0] >= 200, int(keep.sum())

    def f_points(p):
        comp.set_transforms(pose_matrices(params), batch_dim=(A,))
        return comp(p)

    def f_pose(q):
        comp.set_transforms(pose_matrices(q), batch_dim=(A,))
        return comp(pts)

    assert torch.autograd.gradcheck(f_points, (pts.clone().requires_grad_(),), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)
    assert torch.autograd.gradcheck(f_pose, (params.clone().requires_grad_(),), eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def test_composed_float32_matches_float64_restatement_c3_size(cached):
    """float32 HIP backward vs ComposedOpForOp with autograd in float64, A = 20 x P = 16,384, 8 leaves."""
    S, A, P = 8, 20, 16384
    m = W.random_rigid(S * A, seed=9, trans=0.2).cuda()
    comp = pv.ComposedSDF([cached] * S, None)
    pts = W.c3_points(P, seed=2)
    m64 = m.double()
    with torch.no_grad():
        best, ok = composed_decisions([cached] * S, m64, pts.double(), A)
    assert ok.float().mean() > 0.9
    g = torch.Generator(device="cuda").manual_seed(3)
    wv = torch.randn(A, P, generator=g, device="cuda", dtype=torch.float64) * ok
    wg = torch.randn(A, P, 3, generator=g, device="cuda", dtype=torch.float64) * ok.unsqueeze(-1)

    mm = m.clone().requires_grad_()
    comp.set_transforms(mm, batch_dim=(A,))
    p32 = pts.clone().requires_grad_()
    val, grad = comp(p32)
    with torch.no_grad():  # forward decisions first: the values agree with the restatement where it is decided
        ref_val, _ = ComposedOpForOp([ref_leaf(cached, "cuda")] * S, m64, batch=A)(pts.double())
        assert torch.allclose(val.double()[ok], ref_val[ok], atol=1e-5)
    ((val.double() * wv).sum() + (grad.double() * wg).sum()).backward()

    m64g = m64.clone().requires_grad_()
    p64 = pts.double().requires_grad_()
    rv, rg = ComposedOpForOp([ref_leaf(cached, "cuda")] * S, m64g, batch=A)(p64)
    ((rv * wv).sum() + (rg * wg).sum()).backward()
    dp, dp_ref = p32.grad.double(), p64.grad
    dm, dm_ref = mm.grad.double(), m64g.grad
    assert torch.allclose(dp, dp_ref, rtol=1e-3, atol=1e-3 * dp_ref.abs().max()), float((dp - dp_ref).abs().max())
    # matrix entries: compare along the rigid parametrisation -- the rotation part through the tangent R^T dR (skew part) and
    # the translation column; the reference's inverse() and the kernels' transpose differ off the rigid manifold only
    R = m64[:, :3, :3]
    skew = lambda d: (R.transpose(-1, -2) @ d[:, :3, :3]) - (R.transpose(-1, -2) @ d[:, :3, :3]).transpose(-1, -2)
    scale = dm_ref[:, :3, :].abs().max()
    assert torch.allclose(dm[:, :3, 3], dm_ref[:, :3, 3], atol=2e-3 * scale)
    assert torch.allclose(skew(dm), skew(dm_ref), atol=2e-3 * scale)
    # and all 12 entries of every matrix (row 3 exactly zero) against the decision-conditioned float64 VJP, whose transpose
    # form is the contract for raw matrix entries: a worst-case rounding bound (tests/test_autograd_edges_gpu.py)
    from oracle import conditioned_vjp as cv
    r = cv.composed_vjp([H.oracle_grid_from_cached(cached)] * S, m.cpu().numpy(), A, pts.cpu().numpy(), wv.cpu(), wg.cpu())
    assert torch.equal(mm.grad[:, 3], torch.zeros_like(mm.grad[:, 3]))
    ok, worst, _ = cv.within_bound(mm.grad, r["dtf"], r["dtf_mag"], 2.0 ** -24, -(-P // 1024) + 14, c=4.0)
    assert ok, worst
    ok, worst, _ = cv.within_bound(p32.grad, r["dpoints"], r["dpoints_mag"], 2.0 ** -24, A, c=4.0)
    assert ok, worst


def test_composed_backward_is_reproducible(cached):
    S, A, P = 8, 16, 50000
    m = W.random_rigid(S * A, seed=12, trans=0.2).cuda().requires_grad_()
    comp = pv.ComposedSDF([cached] * S, None)
    pts = W.c3_points(P, seed=5).requires_grad_()
    outs = []
    for _ in range(2):
        comp.set_transforms(m, batch_dim=(A,))
        v, g = comp(pts)
        dm, dp = torch.autograd.grad(v.sum() + (g * 0.5).sum(), (m, pts))
        outs.append((dm, dp))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with torch.no_grad():  # the pinned forward gives the same bits as every other dispatch
        v0, g0 = comp(pts.detach())
    comp.group_points = True
    v1, g1 = comp(pts.detach())
    assert torch.equal(v.detach(), v0) and torch.equal(g.detach(), g0) and torch.equal(v0, v1) and torch.equal(g0, g1)


def test_no_grad_paths_unchanged_and_double_backward_raises(cached):
    pts = W.c2_points(cached, 5000, seed=1)
    v0, g0 = cached(pts)
    assert v0.grad_fn is None and g0.grad_fn is None
    p = pts.clone().requires_grad_()
    with torch.no_grad():
        v1, g1 = cached(p)
    assert v1.grad_fn is None and torch.equal(v0, v1) and torch.equal(g0, g1)
    v2, g2 = cached(p)
    assert torch.equal(v0, v2.detach()) and torch.equal(g0, g2.detach())
    with pytest.raises(RuntimeError):
        (dp,) = torch.autograd.grad(v2.sum(), p, create_graph=True)
        dp.sum().backward()
    comp = W.build_c3(cached)
    cp = W.c3_points(3000)
    cv, cg = comp(cp)
    assert cv.grad_fn is None and not comp._tf_grad


# ---------------------------------------------------------------- robot
def robot_reference_loss(robot, q, pts, margin, mask):
    """The issue's loss through the float64 torch restatement (forward kinematics + ComposedOpForOp)."""
    A = q.shape[0]
    stack = robot._stack_torch(q)
    leaves = [ref_leaf(c, "cuda") for c in robot.sdf.sdfs]
    v, _ = ComposedOpForOp(leaves, stack, batch=A)(pts)
    return (((margin - v).clamp(min=0) ** 2) * mask).sum()


def test_robot_gradient_to_q_matches_restatement(robot):
    A, P, margin = 6, 4000, 0.05
    q = W.c4_joint_configs(A, seed=4).cuda()
    pts = W.c4_points(P, seed=6)
    with torch.no_grad():
        best, ok = composed_decisions(robot.sdf.sdfs, robot._stack_torch(q.double()), pts.double(), A)
    assert ok.float().mean() > 0.9
    qg = q.clone().requires_grad_()
    robot.set_joint_configuration(qg)
    val, grad = robot(pts)
    assert val.grad_fn is not None
    (((margin - val).clamp(min=0) ** 2) * ok).sum().backward()
    q64 = q.double().requires_grad_()
    robot_reference_loss(robot, q64, pts.double(), margin, ok).backward()
    assert qg.grad is not None and torch.isfinite(qg.grad).all()
    assert torch.allclose(qg.grad.double(), q64.grad, rtol=2e-3, atol=2e-3 * q64.grad.abs().max()), (qg.grad, q64.grad)
    robot.set_joint_configuration(q)  # leave the fixture without a graph


def test_robot_c4_size_backward(robot):
    A, P, margin = 200, 262144, 0.05
    q = W.c4_joint_configs(A, seed=0).cuda()
    pts = W.c4_points(P)
    qg = q.clone().requires_grad_()
    robot.set_joint_configuration(qg)
    val, _ = robot(pts)
    k = 3  # the float64 recomputation on a slice of configurations: dq[a] depends on configuration a only
    with torch.no_grad():
        _, ok = composed_decisions(robot.sdf.sdfs, robot._stack_torch(q[:k].double()), pts.double(), k)
    mask = torch.ones(A, P, device="cuda")
    mask[:k] = ok
    (((margin - val).clamp(min=0) ** 2) * mask).sum().backward()
    assert torch.isfinite(qg.grad).all()
    q64 = q[:k].double().requires_grad_()
    robot_reference_loss(robot, q64, pts.double(), margin, ok).backward()
    assert torch.allclose(qg.grad[:k].double(), q64.grad, rtol=2e-3, atol=2e-3 * q64.grad.abs().max())
    robot.set_joint_configuration(q)


# ---------------------------------------------------------------- chamfer
def test_grid_chamfer_gradient_to_pose(cached):
    B, N, scale = 6, 3000, 1000.0
    params = torch.cat((torch.randn(B, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 0.1,
                        torch.randn(B, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)), dim=1).cuda()
    pts = W.c2_points(cached, N, seed=8, margin=0.2).double()
    with torch.no_grad():
        m = pose_matrices(params)
        x = pts.unsqueeze(0) @ m[:, :3, :3].transpose(-1, -2) + m[:, None, :3, 3]
        keep = stable(cached, x).all(0)
    pts = pts[keep].contiguous()
    assert pts.shape[0] >= 1500

    pg = params.clone().requires_grad_()
    err = pv.batch_chamfer_dist(pose_matrices(pg), pts.float(), obj_sdf=cached, scale=scale)
    assert err.grad_fn is not None
    err.sum().backward()

    p64 = params.clone().requires_grad_()
    m64 = pose_matrices(p64)
    x = pts.float().double().unsqueeze(0) @ m64[:, :3, :3].transpose(-1, -2) + m64[:, None, :3, 3]
    d, _ = ref_leaf(cached, "cuda")(x.reshape(-1, 3))
    ((scale * d.reshape(B, -1)) ** 2).mean(dim=-1).sum().backward()
    assert torch.allclose(pg.grad, p64.grad, rtol=2e-3, atol=2e-3 * p64.grad.abs().max()), (pg.grad, p64.grad)
