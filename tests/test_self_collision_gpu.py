"""-m gpu: ComposedSDF.leaf_pair_distance / RobotSDF.self_collision_distance (csrc/leaf_pair.hip) against the contract of
include/pvamd.h "Leaf-pair distance": the pair transforms against a C restatement (tests/leaf_pair_ref.c) and a float64 rigid
product; every pair bit-equal to the one-leaf min_over_points under the pair transform; ties, NaN, signed zero; geometry on the
synthetic arm and on a folded three-link arm; the generic path; autograd to q; reproducibility, graph capture, peak memory."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import mesh_io
from tests import c_ref
from tests.test_interp_gpu import build_robot
from tests.test_min_over_points_gpu import restated_argmin, same_bits

pytestmark = pytest.mark.gpu
S = 8


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def robot():
    return W.build_c4()


@pytest.fixture(scope="module")
def robot_tri():
    return build_robot(interpolation="trilinear")


@pytest.fixture(scope="module")
def ref_lib():
    return c_ref.load("leaf_pair_ref")


def leaf_sets(sizes, seed):
    """One point set per leaf in that leaf's frame, around the arm's link ellipsoid (0.06 x 0.06 x 0.11 about z = 0.09)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor([-0.1, -0.1, -0.05]), torch.tensor([0.1, 0.1, 0.25])
    return [(lo + (hi - lo) * torch.rand(n, 3, generator=g)).cuda() for n in sizes]


RAGGED = [1, 63, 4097, 9000, 256, 300, 17, 1000]  # one point, a partial wave, just above one chunk, above two chunks, ...
ALL_PAIRS = torch.tensor([[s, t] for s in range(S) for t in range(S) if s != t], dtype=torch.int64)


def one_leaf_expected(comp, C, k, s, pts):
    """ComposedSDF([sdfs[s]], C[:, k]).min_over_points(pts): the contract's right-hand side."""
    A = C.reshape(-1, C.shape[-3], 4, 4).shape[0]
    one = pv.ComposedSDF([comp.sdfs[s]], None)
    one.set_transforms(C.reshape(A, -1, 4, 4)[:, k].contiguous(), batch_dim=comp.tsf_batch, known_rigid=True)
    return one.min_over_points(pts)


def check_pairs(comp, pts, pairs, dtype):
    res = comp.leaf_pair_distance(pts, pairs)
    assert isinstance(res, pv.LeafPairDistance)
    batch = tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()
    K = pairs.shape[0]
    assert res.values.shape == batch + (K,) and res.indices.shape == batch + (K,) and res.gradients.shape == batch + (K, 3)
    assert res.values.dtype == dtype and res.gradients.dtype == dtype and res.indices.dtype == torch.int64
    C = comp.leaf_pair_transforms(pairs, dtype=dtype)
    for k, (s, t) in enumerate(pairs.tolist()):
        e = one_leaf_expected(comp, C, k, s, pts[t].to(dtype))
        assert torch.equal(res.indices[..., k].cpu(), e.indices.cpu()), (k, s, t)
        assert same_bits(res.values[..., k].cpu().numpy(), e.values.cpu().numpy()), (k, s, t)
        assert same_bits(res.gradients[..., k, :].cpu().numpy(), e.gradients.cpu().numpy()), (k, s, t)
    return res


# ---------------------------------------------------------------- 1. pair transforms
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_pair_transforms_bits_and_rigid_product(robot, ref_lib, dtype):
    A = 7
    robot.set_joint_configuration(W.c4_joint_configs(A, seed=2).cuda())
    pairs = ALL_PAIRS
    C = robot.sdf.leaf_pair_transforms(pairs, dtype=dtype)
    assert C.shape == (A, len(pairs), 4, 4) and C.dtype == dtype
    stack = robot.sdf._tf_matrix.detach().float().cpu().to(dtype).contiguous().numpy()  # the exact widening in float64
    npdt = np.float32 if dtype == torch.float32 else np.float64
    out = np.zeros((len(pairs), A, 4, 4), npdt)
    p = np.ascontiguousarray(pairs.numpy())
    fn = ref_lib.pair_transforms_f32 if dtype == torch.float32 else ref_lib.pair_transforms_f64
    fn(stack.ctypes.data_as(ctypes.c_void_p), S, A, p.ctypes.data_as(ctypes.c_void_p), len(pairs), out.ctypes.data_as(ctypes.c_void_p))
    got = C.transpose(0, 1).cpu().numpy()
    assert same_bits(got, out)
    # within a few ulp of the float64 product Ms @ rigid_inverse(Mt)
    st = stack.astype(np.float64).reshape(S, A, 4, 4)
    Ms, Mt = st[p[:, 0]], st[p[:, 1]]
    inv = np.zeros_like(Mt)
    inv[..., :3, :3] = np.swapaxes(Mt[..., :3, :3], -1, -2)
    inv[..., :3, 3] = -np.einsum("...ij,...j->...i", inv[..., :3, :3], Mt[..., :3, 3])
    inv[..., 3, 3] = 1
    ref = Ms @ inv
    eps = np.finfo(npdt).eps
    scale = 1 + np.abs(Ms[..., :, 3:4]).max() + np.abs(Mt[..., :3, 3]).max()
    assert np.abs(got.astype(np.float64) - ref).max() <= 8 * eps * scale
    # the robot method is the composition's
    assert torch.equal(robot.link_pair_transforms(pairs), robot.sdf.leaf_pair_transforms(pairs))


# ---------------------------------------------------------------- 2. every pair against the one-leaf reduction
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("A", [1, 7, 200])
def test_bit_equal_to_one_leaf_min_over_points(robot, robot_tri, tri, dtype, A):
    r = robot_tri if tri else robot
    q = W.c4_joint_configs(A, seed=A).cuda()
    r.set_joint_configuration(q[0] if A == 1 else q)
    pts = [p.to(dtype) for p in leaf_sets(RAGGED, seed=A)]
    check_pairs(r.sdf, pts, ALL_PAIRS, dtype)


def test_robot_methods_are_the_compositions(robot):
    robot.set_joint_configuration(W.c4_joint_configs(5, seed=9).cuda())
    robot.set_self_collision_points(num_points=200, seed=3)
    pairs = robot.self_collision_pairs()
    assert pairs.shape == (42, 2)
    res = robot.self_collision_distance()
    ref = robot.sdf.leaf_pair_distance(robot._sc_points, pairs)
    for x, y in zip(res, ref):
        assert torch.equal(x, y)
    assert all(p.shape == (200, 3) for p in robot._sc_points)
    check_pairs(robot.sdf, robot._sc_points, pairs, torch.float32)
    sub = robot.self_collision_distance(pairs[:3])
    assert torch.equal(sub.values, res.values[:, :3])


# ---------------------------------------------------------------- 3. ties, NaN, signed zero
def deepest_voxel_centre(c):
    v = c._view
    k = int(torch.argmin(c._packed[:, 0]))
    ijk = np.unravel_index(k, tuple(v.shape))
    return [float(v.dmin[d]) + ijk[d] * float(v.dres[d]) for d in range(3)], k


def identity_pair(leaf0, leaf1, A=2):
    m = torch.eye(4).repeat(2 * A, 1, 1)
    comp = pv.ComposedSDF([leaf0, leaf1], None)
    comp.set_transforms(m.cuda(), batch_dim=(A,))
    return comp


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_ties_nan_and_signed_zero(tri):
    leaf = W.build_c2_cache()
    if tri:
        leaf.interpolation = "trilinear"
    other = W.build_c2_cache()
    comp = identity_pair(leaf, other)
    centre, k = deepest_voxel_centre(leaf)
    res = float(leaf._view.dres[0])
    g = torch.Generator().manual_seed(5)
    c = torch.tensor(centre, dtype=torch.float32)
    cluster = c + (torch.rand(500, 3, generator=g) - 0.5) * (0.2 * res)
    if tri:  # interpolated values differ inside a voxel: exact duplicates make the ties
        cluster = c.view(1, 3).repeat(500, 1)
    far = W.c3_points(700, seed=6).cpu()
    pts = [torch.zeros(0, 3).cuda(), torch.cat((far, cluster, cluster)).cuda()]
    pairs = torch.tensor([[0, 1]])
    r = check_pairs(comp, pts, pairs, torch.float32)
    v, _ = leaf(pts[1])
    assert int((v == v.min()).sum()) > 1 and int(r.indices[0, 0]) == int(restated_argmin(v.view(1, -1).cpu().numpy())[0])
    # a NaN record: the minimum is NaN, at the first point that reads it
    with torch.no_grad():
        leaf._packed[k, 0] = float("nan")
    cpts = [pts[0], torch.cat((far[:100].cuda(), c.cuda().view(1, 3).repeat(3, 1)))]
    r = check_pairs(comp, cpts, pairs, torch.float32)
    assert torch.isnan(r.values).all() and (r.indices == 100).all()
    if tri:
        return
    # -0.0 / +0.0: every record 1.0 except two voxels holding -0.0 and +0.0 -- they tie, the smaller index wins
    with torch.no_grad():
        leaf._packed[:, 0] = 1.0
        leaf._packed[k, 0] = -0.0
        leaf._packed[k + 1, 0] = 0.0
    v = leaf._view
    ijk2 = np.unravel_index(k + 1, tuple(v.shape))
    c2 = [float(v.dmin[d]) + ijk2[d] * float(v.dres[d]) for d in range(3)]
    z = torch.tensor([c2, centre, c2, centre], dtype=torch.float32, device="cuda")
    for order in (z, z.flip(0)):
        r = check_pairs(comp, [pts[0], order], pairs, torch.float32)
        assert (r.indices == 0).all() and (r.values == 0.0).all()


# ---------------------------------------------------------------- 4. geometry
def test_straight_arm_default_pairs_positive(robot, robot_tri):
    for r in (robot, robot_tri):
        r.set_joint_configuration(torch.zeros(7).cuda())
        r.set_self_collision_points(num_points=256)
        res = r.self_collision_distance()
        assert res.values.shape == (42,)
        assert (res.values > 0).all(), res.values


FOLD = 2.6  # radians at both joints: link 2 folds back through link 0


def folded_arm(tmp, **kw):
    m = mesh_io.uv_sphere_mesh(1.0, 24, 12, scale=(0.06, 0.06, 0.11), center=(0, 0, 0.09))
    parts = ['<robot name="fold">']
    for i in range(3):
        mesh_io.save_obj(os.path.join(tmp, f"l{i}.obj"), m)
        parts.append(f'<link name="l{i}"><visual><geometry><mesh filename="l{i}.obj"/></geometry></visual></link>')
    for i in range(2):
        parts.append(f'<joint name="j{i}" type="revolute"><parent link="l{i}"/><child link="l{i + 1}"/>'
                     f'<origin xyz="0 0 0.18"/><axis xyz="0 1 0"/></joint>')
    parts.append("</robot>")
    chain = pv.build_chain_from_urdf("\n".join(parts))
    return pv.RobotSDF(chain, path_prefix=tmp, **kw)


def test_folded_arm_interpenetrates():
    with tempfile.TemporaryDirectory() as tmp:
        r = folded_arm(tmp, link_sdf_cls=pv.cache_link_sdf_factory(0.01, 0.1, device="cuda", cache_path=None))
    assert r.self_collision_pairs().tolist() == [[0, 2], [2, 0]]
    r.set_joint_configuration(torch.tensor([[0.0, 0.0], [FOLD, FOLD]]).cuda())
    r.set_self_collision_points(num_points=512)
    res = r.self_collision_distance()
    assert (res.values[0] > 0).all() and (res.values[1] < 0).all(), res.values
    # the sign agrees with the mesh at the witness point, mapped into leaf s's frame by the pair transform
    C = r.link_pair_transforms()
    for k, (s, t) in enumerate(r.self_collision_pairs().tolist()):
        for a in range(2):
            p = r._sc_points[t][int(res.indices[a, k])]
            x = C[a, k, :3, :3] @ p + C[a, k, :3, 3]
            v, _ = pv.MeshSDF(r.link_factories[s])(x.view(1, 3))
            assert (float(v[0]) < 0) == (a == 1), (a, k, float(v[0]), float(res.values[a, k]))


# ---------------------------------------------------------------- 5. the generic path
def test_generic_path_same_contract(robot, robot_tri):
    with tempfile.TemporaryDirectory() as tmp:
        mesh_robot = pv.RobotSDF(W.synthetic_arm(tmp), path_prefix=tmp)  # MeshSDF links
    mesh_robot.set_joint_configuration(W.c4_joint_configs(3, seed=21).cuda())
    assert mesh_robot.sdf._fused_mode() is None
    pts = leaf_sets([40, 1, 63, 20, 33, 7, 50, 12], seed=22)
    pairs = mesh_robot.self_collision_pairs()
    check_pairs(mesh_robot.sdf, pts, pairs, torch.float32)
    # mixed interpolation: leaves alternate nearest / trilinear under the C4 stack
    robot.set_joint_configuration(W.c4_joint_configs(4, seed=23).cuda())
    mixed = pv.ComposedSDF([(robot_tri if s % 2 else robot).sdf.sdfs[s] for s in range(S)], None)
    mixed.set_transforms(robot.sdf._tf_matrix, batch_dim=(4,), known_rigid=True)
    assert mixed._fused_mode() is None
    check_pairs(mixed, leaf_sets(RAGGED[:2] + [300] * 6, seed=24), ALL_PAIRS, torch.float32)


# ---------------------------------------------------------------- 6. autograd
def pair_transforms64(stack, pairs):
    """Item 1 restated in float64 torch (differentiable): stack (S, A, 4, 4) -> (K, A, 4, 4)."""
    Ms, Mt = stack[pairs[:, 0]], stack[pairs[:, 1]]
    R = Ms[..., :3, :3] @ Mt[..., :3, :3].transpose(-1, -2)
    t = Ms[..., :3, 3] - (R @ Mt[..., :3, 3:4]).squeeze(-1)
    return torch.cat((R, t.unsqueeze(-1)), dim=-1)


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_dq_matches_autograd_through_one_leaf_reductions(robot, robot_tri, tri):
    """q.grad of values.clamp_max(m).sum() against: per pair, autograd through the one-leaf min_over_points w.r.t. its transform
    (the kernel's C, decisions held fixed), chained to q through a float64 torch restatement of the pair transform and the
    chain.  Stated bound: 1e-4 of the largest |dq| (the pair-transform VJP runs in float32 in the kernel)."""
    r = robot_tri if tri else robot
    A, m = 6, 0.3
    q0 = W.c4_joint_configs(A, seed=31).cuda()
    r.set_self_collision_points(num_points=256, seed=1)
    pairs = r.self_collision_pairs()
    q = q0.clone().requires_grad_()
    r.set_joint_configuration(q)
    res = r.self_collision_distance()
    res.values.clamp_max(m).sum().backward()
    got = q.grad.detach().double().cpu()
    # reference
    r.set_joint_configuration(q0)
    C = r.link_pair_transforms().detach()  # (A, K, 4, 4), the kernel's bits
    dC = torch.zeros((len(pairs), A, 4, 4), dtype=torch.float64)
    for k, (s, t) in enumerate(pairs.tolist()):
        Ck = C[:, k].contiguous().requires_grad_()
        one = pv.ComposedSDF([r.sdf.sdfs[s]], None)
        one.set_transforms(Ck, batch_dim=(A,), known_rigid=True)
        e = one.min_over_points(r._sc_points[t])
        assert torch.equal(e.indices, res.indices[:, k])
        (g,) = torch.autograd.grad(e.values.clamp_max(m).sum(), Ck)
        dC[k] = g.double().cpu()
    q64 = q0.double().cpu().requires_grad_()
    stack = r._stack_torch(q64).reshape(S, A, 4, 4)
    C64 = pair_transforms64(stack, pairs)
    (ref,) = torch.autograd.grad(C64, q64, dC[..., :3, :])
    bound = 1e-4 * float(ref.abs().max()) + 1e-7
    assert float(ref.abs().max()) > 0
    assert float((got - ref).abs().max()) <= bound, (got, ref)
    # two backward calls give the same bits
    q2 = q0.clone().requires_grad_()
    r.set_joint_configuration(q2)
    r.self_collision_distance().values.clamp_max(m).sum().backward()
    assert torch.equal(q2.grad, q.grad)


def witness_cells(r, res, pairs):
    """Per (a, k): the voxel of leaf s's grid that the witness falls in (or "out" of the grid range) -- the piece of the
    piecewise-trilinear field the derivative is taken on."""
    C = r.sdf.leaf_pair_transforms(pairs, dtype=torch.float64).cpu()
    out = []
    for a in range(C.shape[0]):
        row = []
        for k, (s, t) in enumerate(pairs.tolist()):
            p = r._sc_points[t][int(res.indices[a, k])].cpu()
            x = C[a, k, :3, :3] @ p + C[a, k, :3, 3]
            v = r.sdf.sdfs[s]._view
            f = [(float(x[d]) - float(v.dmin[d])) / float(v.dres[d]) for d in range(3)]
            inside = all(0 <= f[d] <= v.shape[d] - 1 for d in range(3))
            row.append(tuple(int(np.floor(c)) for c in f) if inside else "out")
        out.append(row)
    return out


def test_trilinear_central_difference(robot_tri):
    """Away from decision edges (same witness, same voxel at q +- h) the q gradient of the summed values is the float64 central
    difference.  Stated bound: 2e-3 + 1e-2 |fd| (the stack is float32: its rounding over 2h is ~1e-4 per pair)."""
    r = robot_tri
    A, h = 3, 5e-4
    pairs = r.self_collision_pairs()[::10]  # a few pairs: fewer voxel faces crossed within h
    q0 = W.c4_joint_configs(A, seed=41).cuda()
    r.set_self_collision_points([p.double() for p in leaf_sets([256] * S, seed=42)])
    q = q0.clone().requires_grad_()
    r.set_joint_configuration(q)
    res = r.self_collision_distance(pairs)
    assert res.values.dtype == torch.float64
    res.values.sum().backward()
    r.set_joint_configuration(q0)
    cells0 = witness_cells(r, res, pairs)
    checked = 0
    for j in range(7):
        side = []
        for sign in (1, -1):
            qs = q0.clone()
            qs[:, j] += sign * h
            r.set_joint_configuration(qs)
            rs = r.self_collision_distance(pairs)
            side.append((rs, witness_cells(r, rs, pairs)))
        (rp, cp), (rm, cm) = side
        for a in range(A):
            if not (torch.equal(rp.indices[a], res.indices[a]) and torch.equal(rm.indices[a], res.indices[a]) and
                    cp[a] == cells0[a] and cm[a] == cells0[a]):
                continue  # a decision edge within h: not a derivative
            fd = float((rp.values[a].sum() - rm.values[a].sum()) / (2 * h))
            assert abs(fd - float(q.grad[a, j])) <= 2e-3 + 1e-2 * abs(fd), (a, j, fd, float(q.grad[a, j]))
            checked += 1
    assert checked >= 5


# ---------------------------------------------------------------- 7. reproducibility, graph capture, memory
def test_reproducible_graph_capture_and_memory(robot):
    A = 200
    robot.set_joint_configuration(W.c4_joint_configs(A, seed=51).cuda())
    robot.set_self_collision_points(num_points=256, seed=2)
    a = robot.self_collision_distance()
    b = robot.self_collision_distance()
    for x, y in zip(a, b):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    robot.self_collision_distance()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 4 << 20
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = robot.self_collision_distance()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, cap):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    # sets above one chunk take the two-pass route: also reproducible
    pts = leaf_sets(RAGGED, seed=52)
    c = robot.sdf.leaf_pair_distance(pts, ALL_PAIRS)
    d = robot.sdf.leaf_pair_distance(pts, ALL_PAIRS)
    for x, y in zip(c, d):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
