"""-m gpu: ComposedSDF.leaf_pair_hinge / RobotSDF.self_collision_hinge (csrc/leaf_pair.hip) against the contract of
include/pvamd.h "Leaf-pair hinge": every pair bit-equal to the one-leaf hinge_over_points under the pair transform (single- and
two-pass routes); a record at the margin and a NaN record; geometry on the synthetic and folded arms; the stack gradient
against the one-leaf hinge's own backward; autograd to q; the generic path; reproducibility, graph capture, peak memory."""
import tempfile

import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from tests.test_min_over_points_gpu import same_bits
from tests.test_self_collision_gpu import (ALL_PAIRS, FOLD, RAGGED, S, deepest_voxel_centre, folded_arm, identity_pair,
                                           leaf_sets, pair_transforms64)
from tests.test_interp_gpu import build_robot

pytestmark = pytest.mark.gpu
GRAD_MARGIN = 0.2  # wider than the grid padding: nearest-leaf points in the bounding-box branch carry a derivative


@pytest.fixture(scope="module")
def robot():
    return W.build_c4()


@pytest.fixture(scope="module")
def robot_tri():
    return build_robot(interpolation="trilinear")


def one_leaf(comp, C, k, s):
    """ComposedSDF([sdfs[s]], C[:, k]): the contract's right-hand side.  C: B + (K, 4, 4)."""
    A = C.reshape(-1, C.shape[-3], 4, 4).shape[0]
    one = pv.ComposedSDF([comp.sdfs[s]], None)
    one.set_transforms(C.reshape(A, -1, 4, 4)[:, k].contiguous(), batch_dim=comp.tsf_batch, known_rigid=True)
    return one


def check_pairs(comp, pts, pairs, margin, power, dtype):
    res = comp.leaf_pair_hinge(pts, pairs, margin, power)
    assert isinstance(res, pv.LeafPairHinge)
    batch = tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()
    K = pairs.shape[0]
    assert res.values.shape == batch + (K,) and res.counts.shape == batch + (K,)
    assert res.values.dtype == dtype and res.counts.dtype == torch.int64
    C = comp.leaf_pair_transforms(pairs, dtype=dtype)
    for k, (s, t) in enumerate(pairs.tolist()):
        e = one_leaf(comp, C, k, s).hinge_over_points(pts[t].to(dtype), margin, power)
        assert same_bits(res.values[..., k].cpu().numpy(), e.values.cpu().numpy()), (k, s, t)
        assert torch.equal(res.counts[..., k].cpu(), e.counts.cpu()), (k, s, t)
    return res


# ---------------------------------------------------------------- 1. every pair against the one-leaf hinge
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("A", [1, 7, 200])
def test_bit_equal_to_one_leaf_hinge(robot, robot_tri, tri, dtype, A):
    r = robot_tri if tri else robot
    q = W.c4_joint_configs(A, seed=A).cuda()
    r.set_joint_configuration(q[0] if A == 1 else q)
    pts = [p.to(dtype) for p in leaf_sets(RAGGED, seed=A)]
    for margin, power in ((0.05, 2), (0.3, 1)) if A == 200 else ((0.05, 1), (0.05, 2), (0.3, 1), (0.3, 2)):
        res = check_pairs(r.sdf, pts, ALL_PAIRS, margin, power, dtype)
        if margin == 0.3:  # some terms positive
            assert (res.values > 0).any() and (res.counts > 0).any()
    # the single-pass route (every set within one chunk)
    small = [p.to(dtype) for p in leaf_sets([1, 63, 256, 4096, 300, 17, 1000, 64], seed=A + 1)]
    check_pairs(r.sdf, small, ALL_PAIRS, 0.3, 2, dtype)


# ---------------------------------------------------------------- 2. the robot wrapper
def test_robot_method_is_the_compositions(robot):
    robot.set_joint_configuration(W.c4_joint_configs(5, seed=9).cuda())
    robot.set_self_collision_points(num_points=200, seed=3)
    pairs = robot.self_collision_pairs()
    res = robot.self_collision_hinge(0.1)
    ref = robot.sdf.leaf_pair_hinge(robot._sc_points, pairs, 0.1)
    for x, y in zip(res, ref):
        assert torch.equal(x, y)
    assert res.values.shape == (5, 42)
    sub = robot.self_collision_hinge(0.1, pairs=pairs[:3])
    assert torch.equal(sub.values, res.values[:, :3]) and torch.equal(sub.counts, res.counts[:, :3])
    p1 = robot.self_collision_hinge(0.1, power=1)
    check_pairs(robot.sdf, robot._sc_points, pairs, 0.1, 1, torch.float32)
    assert torch.equal(p1.counts, res.counts)


# ---------------------------------------------------------------- 3. a record at the margin, a NaN record
def test_value_at_margin_and_nan_record():
    leaf, other = W.build_c2_cache(), W.build_c2_cache()
    comp = identity_pair(leaf, other)
    centre, k = deepest_voxel_centre(leaf)
    rec = float(leaf._packed[k, 0])
    far = W.c3_points(300, seed=6).float().cuda()
    pts = [torch.zeros(0, 3).cuda(), torch.cat((far, torch.tensor([centre], dtype=torch.float32, device="cuda")))]
    pairs = torch.tensor([[0, 1]])
    # the voxel centre reads exactly rec: with margin rec its term is 0 and it is not counted
    r = check_pairs(comp, pts, pairs, rec, 2, torch.float32)
    base = check_pairs(comp, [pts[0], far], pairs, rec, 2, torch.float32)
    assert torch.equal(r.counts, base.counts) and same_bits(r.values.cpu().numpy(), base.values.cpu().numpy())
    # a NaN record: the pair's value is NaN and the point is not counted
    with torch.no_grad():
        leaf._packed[k, 0] = float("nan")
    r = check_pairs(comp, pts, pairs, rec + 1.0, 1, torch.float32)
    assert torch.isnan(r.values).all()
    v, _ = leaf(far)
    assert (r.counts == int((v < rec + 1.0).sum())).all()


# ---------------------------------------------------------------- 4. geometry
def test_straight_arm_is_clear(robot, robot_tri):
    for r in (robot, robot_tri):
        r.set_joint_configuration(torch.zeros(7).cuda())
        r.set_self_collision_points(num_points=256)
        res = r.self_collision_hinge(0.0)
        assert res.values.shape == (42,)
        assert (res.values == 0).all() and (res.counts == 0).all()


def test_folded_arm_has_a_cost():
    with tempfile.TemporaryDirectory() as tmp:
        r = folded_arm(tmp, link_sdf_cls=pv.cache_link_sdf_factory(0.01, 0.1, device="cuda", cache_path=None))
    r.set_joint_configuration(torch.tensor([[0.0, 0.0], [FOLD, FOLD]]).cuda())
    r.set_self_collision_points(num_points=512)
    res = r.self_collision_hinge(0.0)
    assert (res.values[0] == 0).all() and (res.counts[0] == 0).all()
    assert (res.values[1] > 0).all() and (res.counts[1] > 0).all(), res


# ---------------------------------------------------------------- 5. the stack gradient, exactly
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("power", [1, 2])
def test_stack_gradient_is_the_one_leaf_hinge_gradient(tri, power):
    """Leaf t's rows are the identity, so C == Ms and the pair VJP passes dC through (up to the sign of zero): dtf row s is the
    one-leaf hinge's stack gradient under C."""
    leaf, other = W.build_c2_cache(), W.build_c2_cache()
    if tri:  # both leaves: a mixed composition would take the generic path
        leaf.interpolation = "trilinear"
        other.interpolation = "trilinear"
    A = 3
    m = torch.eye(4).repeat(2 * A, 1, 1)
    ang = torch.tensor([0.3, -0.5, 1.1])
    for a in range(A):
        c, s_ = torch.cos(ang[a]), torch.sin(ang[a])
        m[a, :3, :3] = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
        m[a, :3, 3] = torch.tensor([0.02 * a, -0.01, 0.03])
    tfm = m.cuda().requires_grad_()
    comp = pv.ComposedSDF([leaf, other], None)
    comp.set_transforms(tfm, batch_dim=(A,), known_rigid=True)
    assert comp._fused_mode() == ("trilinear" if tri else "nearest")  # the fused kernels, not the generic path
    pts = [torch.zeros(0, 3).cuda(), W.c3_points(1500, seed=7).float().cuda()]  # above one 1024-point backward chunk
    pairs = torch.tensor([[0, 1]])
    res = comp.leaf_pair_hinge(pts, pairs, GRAD_MARGIN, power)
    (g,) = torch.autograd.grad(res.values.sum(), tfm)
    C = comp.leaf_pair_transforms(pairs).detach()
    Ck = C[:, 0].contiguous().requires_grad_()
    one = pv.ComposedSDF([leaf], None)
    one.set_transforms(Ck, batch_dim=(A,), known_rigid=True)
    e = one.hinge_over_points(pts[1], GRAD_MARGIN, power)
    assert same_bits(res.values[:, 0].detach().cpu().numpy(), e.values.detach().cpu().numpy())
    (ge,) = torch.autograd.grad(e.values.sum(), Ck)
    assert torch.equal(g[:A], ge)
    assert float(ge.abs().max()) > 0


# ---------------------------------------------------------------- 6. autograd to q
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_dq_matches_autograd_through_one_leaf_hinges(robot, robot_tri, tri):
    """q.grad of values.sum() against: per pair, autograd through the one-leaf hinge_over_points w.r.t. its transform, chained
    to q through a float64 torch restatement of the pair transform and the chain.  Bound: 1e-4 of the largest |dq|."""
    r = robot_tri if tri else robot
    A, m = 6, GRAD_MARGIN
    q0 = W.c4_joint_configs(A, seed=31).cuda()
    r.set_self_collision_points(num_points=256, seed=1)
    pairs = r.self_collision_pairs()
    q = q0.clone().requires_grad_()
    r.set_joint_configuration(q)
    r.self_collision_hinge(m).values.sum().backward()
    got = q.grad.detach().double().cpu()
    r.set_joint_configuration(q0)
    C = r.link_pair_transforms().detach()
    dC = torch.zeros((len(pairs), A, 4, 4), dtype=torch.float64)
    for k, (s, t) in enumerate(pairs.tolist()):
        Ck = C[:, k].contiguous().requires_grad_()
        one = pv.ComposedSDF([r.sdf.sdfs[s]], None)
        one.set_transforms(Ck, batch_dim=(A,), known_rigid=True)
        (g,) = torch.autograd.grad(one.hinge_over_points(r._sc_points[t], m).values.sum(), Ck)
        dC[k] = g.double().cpu()
    q64 = q0.double().cpu().requires_grad_()
    stack = r._stack_torch(q64).reshape(S, A, 4, 4)
    (ref,) = torch.autograd.grad(pair_transforms64(stack, pairs), q64, dC[..., :3, :])
    assert float(ref.abs().max()) > 0
    assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-7, (got, ref)
    q2 = q0.clone().requires_grad_()
    r.set_joint_configuration(q2)
    r.self_collision_hinge(m).values.sum().backward()
    assert torch.equal(q2.grad, q.grad)


# ---------------------------------------------------------------- 7. the generic path
def test_generic_path_same_contract(robot, robot_tri):
    with tempfile.TemporaryDirectory() as tmp:
        mesh_robot = pv.RobotSDF(W.synthetic_arm(tmp), path_prefix=tmp)  # MeshSDF links
    mesh_robot.set_joint_configuration(W.c4_joint_configs(3, seed=21).cuda())
    assert mesh_robot.sdf._fused_mode() is None
    pts = leaf_sets([40, 1, 63, 20, 33, 7, 50, 12], seed=22)
    check_pairs(mesh_robot.sdf, pts, mesh_robot.self_collision_pairs(), 0.3, 2, torch.float32)
    # mixed interpolation under the C4 stack
    A = 4
    robot.set_joint_configuration(W.c4_joint_configs(A, seed=23).cuda())
    stack = robot.sdf._tf_matrix.detach()
    mixed = pv.ComposedSDF([(robot_tri if s % 2 else robot).sdf.sdfs[s] for s in range(S)], None)
    mixed.set_transforms(stack, batch_dim=(A,), known_rigid=True)
    assert mixed._fused_mode() is None
    sets = leaf_sets(RAGGED[:2] + [300] * 6, seed=24)
    check_pairs(mixed, sets, ALL_PAIRS, 0.3, 1, torch.float32)
    # its stack gradient agrees with the fused path's on a composition both serve (all nearest): float32 bound
    pairs = ALL_PAIRS[::5]
    grads = []
    for fused in (True, False):
        tfm = stack.clone().requires_grad_()
        comp = pv.ComposedSDF([robot.sdf.sdfs[s] for s in range(S)], None)
        comp.set_transforms(tfm, batch_dim=(A,), known_rigid=True)
        if not fused:
            comp._fused_mode = lambda: None
        assert (comp._fused_mode() == "nearest") == fused
        (g,) = torch.autograd.grad(comp.leaf_pair_hinge(sets, pairs, GRAD_MARGIN).values.sum(), tfm)
        grads.append(g)
    scale = float(grads[0].abs().max())
    assert scale > 0 and float((grads[0] - grads[1]).abs().max()) <= 1e-4 * scale


# ---------------------------------------------------------------- 8. reproducibility, graph capture, memory
def test_reproducible_graph_capture_and_memory(robot):
    A = 200
    q = W.c4_joint_configs(A, seed=51).cuda()
    robot.set_joint_configuration(q)
    robot.set_self_collision_points(num_points=256, seed=2)
    a = robot.self_collision_hinge(0.05)
    b = robot.self_collision_hinge(0.05)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and same_bits(a.values.cpu().numpy(), b.values.cpu().numpy())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    robot.self_collision_hinge(0.05)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 4 << 20
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = robot.self_collision_hinge(0.05)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(a.values.cpu().numpy(), cap.values.cpu().numpy()) and torch.equal(a.counts, cap.counts)
    # forward plus backward w.r.t. the stack
    tfm = robot.sdf._tf_matrix.detach().clone().requires_grad_()
    comp = pv.ComposedSDF(list(robot.sdf.sdfs), None)
    comp.set_transforms(tfm, batch_dim=(A,), known_rigid=True)
    comp._leaf_pair_plan(robot._sc_points, robot.self_collision_pairs())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (g1,) = torch.autograd.grad(comp.leaf_pair_hinge(robot._sc_points, robot.self_collision_pairs(), GRAD_MARGIN).values.sum(), tfm)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 16 << 20  # the gradient g1 included
    (g2,) = torch.autograd.grad(comp.leaf_pair_hinge(robot._sc_points, robot.self_collision_pairs(), GRAD_MARGIN).values.sum(), tfm)
    assert torch.equal(g1, g2) and float(g1.abs().max()) > 0
    # sets above one chunk take the two-pass route: also reproducible
    pts = leaf_sets(RAGGED, seed=52)
    c = robot.sdf.leaf_pair_hinge(pts, ALL_PAIRS, 0.3)
    d = robot.sdf.leaf_pair_hinge(pts, ALL_PAIRS, 0.3)
    assert same_bits(c.values.cpu().numpy(), d.values.cpu().numpy()) and torch.equal(c.counts, d.counts)
