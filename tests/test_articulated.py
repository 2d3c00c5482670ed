"""CPU: the surface of pv.joint_normal_equations and pv.refine_joint_configuration (include/pvamd.h "Joint-space normal
equations"), their argument checks, and the float64 restatement tests/articulated_ref.py: the twist Jacobian against central
differences of the reference chain, the factored normal equations against the per-point form, the gradient against a central
difference of the cost, and the Levenberg-Marquardt loop on the scenario the GPU test repeats.  No GPU: every check raises or
returns before a launch."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import articulated as art
from tests import articulated_ref as AR
from tests import fk_ref as R
from tests.test_fk_tree import leaf_radii, tree_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pvamd.h")).read()
NEW_SYMBOLS = ("pvamd_joint_normal_eq_scratch_bytes", "pvamd_joint_normal_eq", "pvamd_chain_twists", "pvamd_joint_assemble",
               "pvamd_joint_lm_step")
EPS = 2.0 ** -52


def leaf_centre(s):
    """The centre of leaf s's ellipsoid in its own frame (tests/test_fk_tree.py::write_robot)."""
    return 0.0, 0.005 * (s % 3), 0.01 * (s % 4)


def ellipsoid_robot(table=R.TREE):
    S = len(R.leaf_links(table))
    return AR.AnalyticRobot(table, [AR.ellipsoid_fn(leaf_centre(s), leaf_radii(s)) for s in range(S)])


def sphere_robot(table=R.TREE):
    """Sphere leaves: the one closed form here whose returned n is the derivative of its value."""
    S = len(R.leaf_links(table))
    return AR.AnalyticRobot(table, [AR.ellipsoid_fn(leaf_centre(s), (0.03 + 0.004 * s,) * 3) for s in range(S)])


def surface_cloud(robot, q_row, per_leaf, seed, jitter=0.0, radii=leaf_radii):
    """per_leaf points on every leaf's ellipsoid surface, placed in the object frame by the float64 chain at q_row."""
    rng = np.random.default_rng(seed)
    T, _ = AR.stack_and_twists(robot.records, robot.origins, robot.axes, np.asarray(q_row, dtype=np.float64)[None], robot.offset_inv)
    out = []
    for s in range(len(robot.leaf_fn)):
        d = rng.standard_normal((per_leaf, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        local = np.asarray(leaf_centre(s)) + d * np.asarray(radii(s))
        m = AR.rigid_inverse(T[0, s])
        out.append(local @ m[:3, :3].T + m[:3, 3])
    pts = np.concatenate(out)
    return pts + rng.uniform(-jitter, jitter, pts.shape) if jitter else pts


def perturbation(table, A, seed):
    """(A, M) fixed-seed offsets of magnitude 0.05 rad (revolute, continuous) and 5 mm (prismatic), random signs."""
    rng = np.random.default_rng(seed)
    M = len(R.joint_names(table))
    d = np.where(rng.random((A, M)) < 0.5, -0.05, 0.05)
    d[:, R.prismatic_columns(table)] *= 0.1
    return d


# the recovery scenario, shared with tests/test_articulated_gpu.py
RECOVERY = dict(A=3, q_seed=5, q_scale=0.4, cloud_seed=6, per_leaf=60, start_seed=7, iterations=10)


def recovery_case():
    q_true = R.draw_q(R.TREE, RECOVERY["A"], RECOVERY["q_scale"], RECOVERY["q_seed"])
    q_true[1:] = q_true[0]  # one observed cloud; the configurations differ in where they start
    start = (q_true + perturbation(R.TREE, RECOVERY["A"], RECOVERY["start_seed"])).astype(np.float32)
    return q_true, start


def header_define(name):
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, re.M).group(1))


def test_exports_header_and_abi():
    assert pv.joint_normal_equations is art.joint_normal_equations
    assert pv.refine_joint_configuration is art.refine_joint_configuration
    assert pv.JointNormalEquations._fields == ("cost", "gradient", "hessian", "counts", "active", "outliers", "leaf_active")
    assert pv.JointRefinement._fields == ("joint_config", "cost", "initial_cost", "accepted")
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert "Joint-space normal equations" in HEADER
    assert header_define("PVAMD_JOINT_MAX") == 32 == _lib.JOINT_MAX
    assert header_define("PVAMD_JOINT_MAX_LEAVES") == 64 == _lib.JOINT_MAX_LEAVES
    assert lib.pvamd_abi_version() == 16 == _lib.ABI_VERSION
    c = ctypes
    assert _lib.SIGNATURES["pvamd_joint_normal_eq"] == (c.c_int, [
        c.c_void_p, c.c_int32, c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_double,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p])
    # the size is the exported function's: 28 sums and 5 counts of 8 bytes per configuration, leaf and chunk = 264 A S chunks
    per = 8 * (_lib.REG_SUMS + _lib.SEM_COUNTS)
    assert per == 264
    assert _lib.joint_normal_eq_scratch_bytes(1, 1, 1) == per == lib.pvamd_joint_normal_eq_scratch_bytes(1, 1, _lib.REG_CHUNK)
    assert _lib.joint_normal_eq_scratch_bytes(3, 12, _lib.REG_CHUNK + 1) == per * 3 * 12 * 2
    assert lib.pvamd_joint_normal_eq_scratch_bytes(0, 1, 5) == 0 and lib.pvamd_joint_normal_eq_scratch_bytes(5, 1, 0) == 0
    import inspect
    source = inspect.getsource(_lib.joint_normal_eq_scratch_bytes)
    assert "load().pvamd_joint_normal_eq_scratch_bytes(" in source and not any(op in source for op in ("//", "*", "+"))


def test_c_entry_points_check_arguments_before_launching():
    lib = _lib.load()
    null, inf = None, math.inf
    ne, tw, asm, step = lib.pvamd_joint_normal_eq, lib.pvamd_chain_twists, lib.pvamd_joint_assemble, lib.pvamd_joint_lm_step
    assert ne(null, 0, 0, null, 2, null, 5, null, null, inf, null, null, null, null) == _lib.E_SHAPE    # S = 0
    assert ne(null, 65, 0, null, 2, null, 5, null, null, inf, null, null, null, null) == _lib.E_SHAPE   # S > 64
    assert ne(null, 3, 0, null, 2, null, 0, null, null, inf, null, null, null, null) == _lib.E_SHAPE    # N = 0
    assert ne(null, 3, 0, null, -1, null, 5, null, null, inf, null, null, null, null) == _lib.E_SHAPE   # A < 0
    assert ne(null, 3, 2, null, 2, null, 5, null, null, inf, null, null, null, null) == -4              # no such leaf mode
    for bad in (0.0, -0.01, math.nan):
        assert ne(null, 3, 0, null, 0, null, 5, null, null, bad, null, null, null, null) == -4          # before A = 0 returns
    assert ne(null, 3, 0, null, 2, null, 5, null, null, 0.01, null, null, null, null) == -1             # NULL pointers
    assert ne(null, 3, 1, null, 0, null, 5, null, null, inf, null, null, null, null) == 0               # A = 0: nothing to do
    assert tw(null, 0, null, 1, 1, null, 1, null, null) == _lib.E_SHAPE and tw(null, 3, null, 1, 33, null, 1, null, null) == _lib.E_SHAPE
    assert tw(null, 3, null, 1, 2, null, 65, null, null) == _lib.E_SHAPE
    assert tw(null, 3, null, 1, 2, null, 1, null, null) == -1
    assert tw(null, 3, null, 0, 2, null, 1, null, null) == 0 and tw(null, 3, null, 4, 0, null, 1, null, null) == 0
    assert asm(null, null, null, 1, 0, 1, null, null, null) == _lib.E_SHAPE and asm(null, null, null, 1, 1, 33, null, null, null) == _lib.E_SHAPE
    assert asm(null, null, null, 1, 1, 1, null, null, null) == -1 and asm(null, null, null, 0, 1, 1, null, null, null) == 0
    ok = (10.0, 0.1, 1e-12, 1e12)
    assert step(1, 33, null, 1, null, null, null, null, null, null, null, *ok, null) == _lib.E_SHAPE
    assert step(-1, 2, null, 1, null, null, null, null, null, null, null, *ok, null) == _lib.E_SHAPE
    for bad in ((1.0, 0.1, 1e-12, 1e12), (10.0, 0.0, 1e-12, 1e12), (10.0, 1.5, 1e-12, 1e12), (10.0, 0.1, 0.0, 1e12),
                (10.0, 0.1, 1.0, 0.5), (10.0, 0.1, 1e-12, inf)):
        assert step(1, 2, null, 1, null, null, null, null, null, null, null, *bad, null) == -4, bad
    assert step(1, 2, null, 2, null, null, null, null, null, null, null, *ok, null) == -4               # first is 0 or 1
    assert step(1, 2, null, 1, null, null, null, null, null, null, null, *ok, null) == -1
    assert step(0, 2, null, 1, null, null, null, null, null, null, null, *ok, null) == 0


def stub_leaf(interpolation="nearest", oob=pv.OutOfBoundsStrategy.BOUNDING_BOX):
    leaf = pv.CachedSDF.__new__(pv.CachedSDF)
    for name, value in (("_dim", 3), ("out_of_bounds_strategy", oob), ("interpolation", interpolation)):
        object.__setattr__(leaf, name, value)
    return leaf


def stub_robot(leaves=None, chain=None, joints=None):
    """A RobotSDF as far as the host-side checks read it: no GPU is needed to make one."""
    robot = pv.RobotSDF.__new__(pv.RobotSDF)
    robot.chain = tree_chain() if chain is None else chain
    robot.joint_names = R.joint_names(R.TREE) if joints is None else joints
    robot.sdf_to_link_name = R.leaf_links(R.TREE)
    robot.sdf = types.SimpleNamespace(sdfs=[stub_leaf() for _ in range(12)] if leaves is None else leaves)
    return robot


@pytest.mark.parametrize("call", [pv.joint_normal_equations, pv.refine_joint_configuration])
def test_argument_errors_raise_before_a_gpu_is_asked_for(call):
    robot, q, cloud = stub_robot(), torch.zeros(3, 8), torch.zeros(5, 3)
    with pytest.raises(TypeError):
        call(pv.SphereSDF(0.1), q, cloud)
    for pts in (torch.zeros(5, 2), torch.zeros(2), torch.empty(0, 3)):
        with pytest.raises(ValueError):
            call(robot, q, pts)
    for bad in (torch.zeros(3, 7), torch.zeros(9), torch.zeros(()), torch.zeros(2, 3, 8)):
        with pytest.raises(ValueError, match="joint_config"):
            call(robot, bad, cloud)
    with pytest.raises(TypeError):
        call(robot, q, cloud, scale=True)
    with pytest.raises(TypeError):
        call(robot, q, cloud, semantics=torch.zeros(5))
    with pytest.raises(ValueError):
        call(robot, q, cloud, semantics=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        call(robot, q, cloud, targets=torch.zeros(4))
    with pytest.raises(TypeError):
        call(robot, q, cloud, huber_delta="0.01")
    for bad in (0.0, -1e-3, math.nan):
        with pytest.raises(ValueError):
            call(robot, q, cloud, huber_delta=bad)
    # the robots that are not served, each named
    mesh_leaf = types.SimpleNamespace()
    with pytest.raises(ValueError, match="leaf 2"):
        call(stub_robot(leaves=[stub_leaf(), stub_leaf(), mesh_leaf] + [stub_leaf()] * 9), q, cloud)
    with pytest.raises(ValueError, match="BOUNDING_BOX"):
        call(stub_robot(leaves=[stub_leaf(oob=pv.OutOfBoundsStrategy.LOOKUP_GT_SDF)] + [stub_leaf()] * 11), q, cloud)
    with pytest.raises(ValueError, match="one interpolation"):
        call(stub_robot(leaves=[stub_leaf("trilinear")] + [stub_leaf()] * 11), q, cloud)
    with pytest.raises(ValueError, match="kinematics.Chain"):
        call(stub_robot(chain=types.SimpleNamespace()), q, cloud)
    with pytest.raises(ValueError, match="at most 64 leaves"):
        call(stub_robot(leaves=[stub_leaf()] * 65), q, cloud)
    with pytest.raises(ValueError, match="at most 32 joints"):
        call(stub_robot(joints=[f"j{k}" for k in range(33)]), torch.zeros(33), cloud)
    # valid arguments get as far as the device, and no further without one
    if not torch.cuda.is_available():
        with pytest.raises((_lib.PvamdError, AttributeError)):
            call(robot, q, cloud)


def test_refinement_argument_errors():
    robot, q, cloud = stub_robot(), torch.zeros(3, 8), torch.zeros(5, 3)
    with pytest.raises(ValueError):
        pv.refine_joint_configuration(robot, q, cloud, iterations=0)
    with pytest.raises(TypeError):
        pv.refine_joint_configuration(robot, q, cloud, iterations=2.0)
    with pytest.raises(ValueError):
        pv.refine_joint_configuration(robot, q, cloud, damping=0.0)
    with pytest.raises(ValueError):
        pv.refine_joint_configuration(robot, q, cloud, damping_up=1.0)
    for bad in (torch.zeros(8), torch.zeros(7, 2), torch.zeros(8, 3)):
        with pytest.raises(ValueError, match="joint_limits"):
            pv.refine_joint_configuration(robot, q, cloud, joint_limits=bad)
    lim = torch.tensor([[-1.0, 1.0]] * 8)
    for row in ([1.0, -1.0], [math.nan, 1.0]):
        bad = lim.clone()
        bad[3] = torch.tensor(row)
        with pytest.raises(ValueError, match="lower <= upper"):
            pv.refine_joint_configuration(robot, q, cloud, joint_limits=bad)
    with pytest.raises(TypeError):
        pv.refine_joint_configuration(robot, q, cloud, joint_limits=torch.zeros((8, 2), dtype=torch.bool))


def test_limits_are_float32_values_inside_the_callers():
    lim = np.array([[-0.1, 0.1], [0.25, 0.25], [-1e-3, 0.3], [0.1, 0.1 + 1e-7]])
    got = art._check_limits(torch.from_numpy(lim), 4)
    assert got.dtype == np.float64 and np.array_equal(got, got.astype(np.float32).astype(np.float64))
    assert (got[:, 0] >= lim[:, 0]).all() and (got[:, 1] <= lim[:, 1]).all() and (got[:, 0] <= got[:, 1]).all()
    assert np.abs(got - lim).max() <= 2.0 ** -24 * np.abs(lim).max() * 2
    assert art._check_limits(None, 4) is None
    with pytest.raises(ValueError, match="no float32 value"):
        art._check_limits(torch.tensor([[0.1, 0.1]], dtype=torch.float64), 1)  # 0.1 is no float32 value


def test_reference_walk_is_the_reference_chain():
    """articulated_ref walks records (what the kernel is given); on the table's float64 origins it is fk_ref.fk64 and
    fk_ref.stack64."""
    records, origins, axes = AR.table_chain(R.TREE)
    assert len(records) == 15 and records == R.expected_records(R.TREE)
    q = R.draw_q(R.TREE, 4, 0.8, seed=3)
    own, _ = R.frame_records(R.TREE)
    want = R.fk64(R.TREE, q)
    for a in range(4):
        world = AR.walk(records, origins, axes, q[a])
        assert np.abs(world[own] - want[:, a]).max() < 1e-14
    offsets = R.visual_offsets64(R.TREE)
    T, _ = AR.stack_and_twists(records, origins, axes, q, np.stack([AR.rigid_inverse(o) for o in offsets]))
    stack = R.stack64(R.TREE, q, offsets).reshape(12, 4, 4, 4)
    assert np.abs(T.transpose(1, 0, 2, 3) - stack).max() < 1e-14


@pytest.mark.parametrize("seed", [1, 2])
def test_twist_jacobian_against_central_differences_of_the_reference_stack(seed):
    """d(T_s)/dq_k T_s^-1 = [w]x, u of column k, from central differences (h = 1e-6) of fk_ref.stack64: within 1e-8 per entry
    (1.7e-10 was measured when the formula was derived; the margin is for other seeds).  Columns of joints that are no ancestor of
    the leaf are exactly zero."""
    robot = ellipsoid_robot()
    q = R.draw_q(R.TREE, 3, 0.8, seed=seed)
    offsets = R.visual_offsets64(R.TREE)
    _, J = AR.stack_and_twists(robot.records, robot.origins, robot.axes, q, robot.offset_inv)
    A, M, S, h = 3, 8, 12, 1e-6
    worst = 0.0
    for k in range(M):
        dq = np.zeros_like(q)
        dq[:, k] = h
        plus = R.stack64(R.TREE, q + dq, offsets).reshape(S, A, 4, 4)
        minus = R.stack64(R.TREE, q - dq, offsets).reshape(S, A, 4, 4)
        base = R.stack64(R.TREE, q, offsets).reshape(S, A, 4, 4)
        for s in range(S):
            for a in range(A):
                # x' = x + dq (w cross x + u):  dT/dq = [[w]x, u] T
                G = ((plus[s, a] - minus[s, a]) / (2 * h)) @ AR.rigid_inverse(base[s, a])
                fd = np.array([G[0, 3], G[1, 3], G[2, 3], G[2, 1], G[0, 2], G[1, 0]])
                worst = max(worst, float(np.abs(fd - J[a, s, :, k]).max()))
    print(f"twist Jacobian against central differences [seed {seed}]: worst entry {worst:.3g}")
    assert worst <= 1e-8
    for s in range(S):
        moving = AR.ancestors(robot.records, s)
        others = [k for k in range(M) if k not in moving]
        assert (J[:, s][:, :, others] == 0.0).all()
        assert (np.abs(J[:, s][:, :, moving]).max(axis=(0, 1)) > 0).all()
    # the table's shape: the torso hangs off a fixed joint (no column), tip_a moves with lift, shoulder, elbow, palm, finger_a
    assert AR.ancestors(robot.records, 0) == [] and AR.ancestors(robot.records, 8) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("options", ["plain", "semantic"])
def test_factored_form_is_the_per_point_form(options):
    """sum_s J_s^T (sums of leaf s) J_s against the sum over points of J_{s(p)}^T j6_p terms (math.fsum), on ellipsoid leaves.
    Per entry |difference| <= (N + 36 S + 64) 2^-52 (|J|^T A |J|), A the per-leaf fsum of the terms' magnitudes: N roundings of a
    leaf's sums at most, 36 S + 64 of the assembly, all relative to the factored magnitudes (J^T j6 can cancel, so the per-point
    magnitudes are no bound)."""
    robot = ellipsoid_robot()
    q = R.draw_q(R.TREE, 2, 0.6, seed=11)
    pts = surface_cloud(robot, q[0], 40, seed=12, jitter=0.01)
    N, S = len(pts), 12
    rng = np.random.default_rng(13)
    kinds = rng.integers(0, 4, N) if options == "semantic" else None
    targets = rng.uniform(-0.02, 0.02, N) if options == "semantic" else None
    delta = 0.01 if options == "semantic" else math.inf
    worst = 0.0
    for a in range(2):
        e = robot.leaf_sums(q[a], pts, kinds, targets, delta)
        assert len(set(e["win"].tolist())) >= (8 if a == 0 else 4)  # several leaves win; the cloud was sampled at q[0]
        cost, g, H = AR.assemble(e["sums"], e["J"])
        mc, mg, mH = AR.assemble_magnitude(e["mags"], e["J"])
        bc, bg, bH = AR.brute_force(e["j6"], e["w"], e["r"], e["win"], e["J"], delta)
        k = (N + 36 * S + 64) * EPS
        for got, want, mag in ((cost, bc, mc), (g, bg, mg), (H, bH, mH)):
            err, bound = np.abs(np.asarray(got) - np.asarray(want)), k * np.asarray(mag)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (options, a, err, bound)
        assert np.array_equal(H, H.T)
        if options == "semantic":
            assert (e["flags"].sum(0) > 0).all()  # every class of pair occurs
    print(f"factored against per-point form [{options}]: worst error / bound = {worst:.3g}")


def test_twice_the_gradient_is_the_derivative_of_the_cost():
    """Sphere leaves (their n is the derivative of their value), points with a clear winner: 2 gradient against a central
    difference of the cost in every joint (h = 1e-6), within 1e-8 |gradient|_inf.  The margin between the winner and the runner-up
    is asserted: 1e-6 rad or m moves a value by at most 1e-6 times the reach of the chain, far below it."""
    robot = sphere_robot()
    q = R.draw_q(R.TREE, 2, 0.6, seed=21)
    cloud = surface_cloud(robot, q[0], 30, seed=22, jitter=0.004, radii=lambda s: (0.03 + 0.004 * s,) * 3)
    h, margin = 1e-6, 1e-3
    for a in range(2):
        T, _ = AR.stack_and_twists(robot.records, robot.origins, robot.axes, q[a][None], robot.offset_inv)
        vals = np.stack([robot.leaf_fn[s](cloud @ T[0, s, :3, :3].T + T[0, s, :3, 3])[0] for s in range(12)])
        two = np.sort(vals, axis=0)[:2]
        pts = cloud[two[1] - two[0] > margin]
        assert len(pts) > 200 and margin > 100 * h * AR.reach(robot.records, robot.origins)
        cost, g, _ = robot.evaluate(q[a], pts)
        fd = np.zeros(8)
        for k in range(8):
            dq = np.zeros(8)
            dq[k] = h
            fd[k] = (robot.evaluate(q[a] + dq, pts)[0][0] - robot.evaluate(q[a] - dq, pts)[0][0]) / (2 * h)
        err = np.abs(2 * g[0] - fd).max()
        print(f"2 gradient against a central difference of the cost [a {a}]: {err:.3g} of |g|_inf {np.abs(g[0]).max():.3g}")
        assert err <= 1e-8 * np.abs(g[0]).max()
        assert (np.abs(g[0]) > 0).sum() >= 5  # most joints are observed by points with a clear winner


def test_step_decisions():
    """The zero step of an unobserved joint, the failed pivot, the strict accept and the clamp."""
    H = np.diag([2.0, 0.0, 3.0])
    st = AR.JointState(q_try=np.array([0.1, 0.2, 0.3]), lam=1e-3)
    AR.lm_step(st, 1.0, np.array([0.2, 0.0, -0.3]), H, True)
    assert st.accepted == 1 and st.dq[1] == 0.0 and st.dq[0] < 0 < st.dq[2] and st.lam == 1e-4
    AR.lm_step(st, 1.0, np.zeros(3), H, False)  # equal cost: not accepted
    assert st.accepted == 1 and st.lam == 1e-3 and np.array_equal(st.q_acc, [0.1, 0.2, 0.3])
    assert np.array_equal(st.q_try, st.q_acc + st.dq)  # a step from the accepted state, with the larger damping
    AR.lm_step(st, math.nan, np.zeros(3), H, False)  # a NaN never accepts
    assert st.accepted == 1
    bad = AR.JointState(q_try=np.array([0.1, 0.2]), lam=1e-3)
    AR.lm_step(bad, 1.0, np.array([1.0, 1.0]), np.array([[1.0, 2.0], [2.0, 1.0]]), True)  # indefinite: a failed pivot
    assert np.array_equal(bad.dq, [0.0, 0.0]) and np.array_equal(bad.q_try, bad.q_acc) and bad.lam == 1e-3
    lim = np.array([[0.0, 0.12], [-1.0, 1.0], [0.0, 0.31]])
    st = AR.JointState(q_try=np.array([0.1, 0.2, 0.3]), lam=1e-3)
    AR.lm_step(st, 1.0, np.array([-2.0, 0.0, -3.0]), H, True, limits=lim)
    assert st.q_try.tolist() == [0.12, 0.2, 0.31]


def test_loop_recovers_the_configuration_on_analytic_leaves():
    """The scenario the GPU test repeats on caches: surface samples of the ellipsoid leaves placed by the float64 chain at q_true,
    a start 0.05 rad / 5 mm off in every joint, ten iterations.  Every configuration accepts at least twice and ends below its
    start; printed, not asserted: how far from q_true it starts and ends."""
    robot = ellipsoid_robot()
    q_true, start = recovery_case()
    pts = surface_cloud(robot, q_true[0], RECOVERY["per_leaf"], RECOVERY["cloud_seed"])
    states, initial = AR.refine(lambda q32: robot.evaluate(q32, pts), start, iterations=RECOVERY["iterations"])
    accepted = [s.accepted for s in states]
    final = np.array([s.cost_acc for s in states])
    before = np.abs(start.astype(np.float64) - q_true).max(axis=1)
    after = np.abs(np.stack([s.q_acc for s in states]) - q_true).max(axis=1)
    print(f"recovery on analytic leaves: accepted {accepted}, cost {initial.tolist()} -> {final.tolist()}, |q - q_true|_inf "
          f"{before.tolist()} -> {after.tolist()}")
    assert all(n >= 2 for n in accepted) and (final < initial).all()
    # with limits that bind one revolute and one prismatic joint, nothing leaves them
    lim = np.array([[-10.0, 10.0]] * 8)
    lim[1] = [start[0, 1] - 0.01, start[0, 1] + 0.01]
    lim[4] = [start[0, 4] - 0.001, start[0, 4] + 0.001]
    lim = art._check_limits(torch.from_numpy(lim), 8)
    states, _ = AR.refine(lambda q32: robot.evaluate(q32, pts), start[:1], iterations=4, limits=lim)
    for qa, _, _ in states[0].history:
        assert (qa >= lim[:, 0]).all() and (qa <= lim[:, 1]).all()
