"""-m gpu: the forward-kinematics kernels of csrc/fk.hip (chain_fk_kernel, configure_chain_kernel) and RobotSDF on a branching
tree with prismatic and fixed joints, links with several mesh visuals, mesh-less frames and a slot order that is not the frame
order -- bit for bit against the CPU oracle fed the sines and cosines the kernel emitted, and within 2e-6 of tests/fk_ref.py, a
float64 reference that does not go through kinematics.Chain.  (The host half: tests/test_fk_tree.py.)

Measured on an MI355X (largest absolute error; every test prints its figures, -s):
    sin / cos against float64, randn * 3:          0.82, 0.90, 0.86, 0.82 x 2^-24 at A = 1, 64, 65, 130
    sin / cos against float64, the wide values:    0.28 x 2^-24 (at |q| = 100 and 10^4; below 2^-30 at the multiples of pi / 2)
    link frames against float64:                   1.1e-7, 2.0e-7, 2.0e-7, 1.9e-7 at A = 1, 64, 65, 130; wide values 1.2e-7
    stack against float64:                         1.3e-7, 2.0e-7, 2.1e-7, 4.1e-7;                        wide values 1.5e-7
    RobotSDF stack against float64:                1.5e-7 (A = 5), 1.7e-7 (2 x 3)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import oracle
from tests import fk_ref as R
from tests import helpers as H
from tests import test_fk_tree as T

pytestmark = pytest.mark.gpu

FK_TOL = T.FK_TOL
SINCOS_TOL = 1e-6   # absolute, against float64 sin / cos of the float32 joint value (the existing configure test's bound)
GUARD = 1024        # floats of sentinel in front of and behind every output buffer
SENTINEL = -7.5


def guarded(n):
    """A device buffer of n floats between two guard bands; everything prefilled with the sentinel."""
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_untouched(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all())


def oracle_fk(raw, q, sn, cn, S, A):
    """oracle_chain_fk on joint_table's bytes with the given sines and cosines: world (F, A, 12), link_world (S * A, 4, 4)."""
    F = len(raw) // C.sizeof(oracle.OracleJoint)
    joints = (oracle.OracleJoint * F).from_buffer_copy(raw)
    M = q.shape[1]
    q, sn, cn = (np.ascontiguousarray(x, dtype=np.float32) for x in (q, sn, cn))
    world = np.zeros((F, A, 12), np.float32)
    lw = np.zeros((S * A, 4, 4), np.float32)
    oracle.load().oracle_chain_fk(joints, C.c_int32(F), C.c_void_p(q.ctypes.data), C.c_void_p(sn.ctypes.data),
                                  C.c_void_p(cn.ctypes.data), C.c_int32(A), C.c_int32(M), C.c_void_p(world.ctypes.data),
                                  C.c_void_p(lw.ctypes.data))
    return world, lw


def run_kernels(raw, q, off_inv, S):
    """pvamd_configure_chain, then pvamd_chain_fk + pvamd_transform_stack on the sines and cosines it emitted, every output
    between guard bands.  q: (A, M) float32 numpy.  Returns the outputs as numpy arrays; asserts the guards."""
    lib = pv._lib.load()
    A, M = q.shape
    F = len(raw) // C.sizeof(pv._lib.JointDesc)
    joints = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda() if M else None
    offd = torch.from_numpy(np.ascontiguousarray(off_inv, dtype=np.float32)).cuda()
    bufs = {name: guarded(n) for name, n in (("sincos", A * M * 2), ("scratch", F * 12 * A), ("lw", S * A * 16),
                                             ("stack", S * A * 16), ("scratch2", F * 12 * A), ("lw2", S * A * 16),
                                             ("stack2", S * A * 16))}
    v = {k: b[1] for k, b in bufs.items()}
    rc = lib.pvamd_configure_chain(pv._lib.ptr(joints), F, pv._lib.ptr(qd), A, M, pv._lib.ptr(offd), S,
                                   pv._lib.ptr(v["sincos"]) if M else pv._lib.ptr(None), pv._lib.ptr(v["scratch"]),
                                   pv._lib.ptr(v["lw"]), pv._lib.ptr(v["stack"]), pv._lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    sincos = v["sincos"].reshape(A, M, 2)
    sin_d, cos_d = sincos[..., 0].contiguous(), sincos[..., 1].contiguous()
    rc = lib.pvamd_chain_fk(pv._lib.ptr(joints), F, pv._lib.ptr(qd), pv._lib.ptr(sin_d if M else None),
                            pv._lib.ptr(cos_d if M else None), A, M, pv._lib.ptr(v["scratch2"]), pv._lib.ptr(v["lw2"]),
                            pv._lib.stream_ptr())
    assert rc == 0
    pv._lib.check(lib.pvamd_transform_stack(pv._lib.ptr(offd), pv._lib.ptr(v["lw2"]), S, A, pv._lib.ptr(v["stack2"]),
                                            pv._lib.stream_ptr()), "pvamd_transform_stack")
    torch.cuda.synchronize()
    for name, (whole, _) in bufs.items():
        assert guards_untouched(whole), f"{name}: written outside the buffer"
    out = {k: t.cpu().numpy() for k, t in v.items()}
    out["sincos"] = out["sincos"].reshape(A, M, 2)
    for k in ("scratch", "scratch2"):
        out[k] = out[k].reshape(F, 12, A)
    for k in ("lw", "lw2", "stack", "stack2"):
        out[k] = out[k].reshape(S * A, 4, 4)
    return out


def check_against_oracle_and_float64(table, raw, leaves, offsets, q, out, label):
    """Everything the kernels wrote: bit for bit the oracle's walk on the emitted sines / cosines (all F x 12 x A scratch values,
    the leaf frames, the stack), the same bits from the two-kernel path, and within 2e-6 of the float64 reference."""
    A, M = q.shape
    S = len(leaves)
    sn, cn = out["sincos"][..., 0], out["sincos"][..., 1]
    assert not (out["sincos"] == SENTINEL).any()
    world, olw = oracle_fk(raw, q, sn, cn, S, A)
    off_inv = np.linalg.inv(offsets).astype(np.float32)
    assert np.array_equal(out["lw"], olw)
    assert np.array_equal(out["scratch"].transpose(0, 2, 1), world)
    assert np.array_equal(out["stack"], oracle.transform_stack(off_inv, olw, S, A))
    assert np.array_equal(out["lw2"], out["lw"]) and np.array_equal(out["scratch2"], out["scratch"])
    assert np.array_equal(out["stack2"], out["stack"])
    own, _ = R.frame_records(table, leaves)
    ref = R.fk64(table, q)
    err_frames = max(np.abs(out["scratch"][i].T.reshape(A, 3, 4) - ref[f, :, :3, :]).max() for f, i in enumerate(own))
    err_lw = np.abs(out["lw"] - R.leaf_world64(table, q, leaves)).max()
    err_stack = np.abs(out["stack"] - R.stack64(table, q, offsets, leaves)).max()
    print(f"{label}: against float64: frames {err_frames:.3e} leaf frames {err_lw:.3e} stack {err_stack:.3e}")
    assert err_frames < FK_TOL and err_lw < FK_TOL and err_stack < FK_TOL
    return err_frames, err_lw, err_stack


def sincos_error(q, sincos):
    """Largest |emitted - float64 sin / cos of the float32 joint value|, absolute."""
    q64 = q.astype(np.float64)
    return max(np.abs(sincos[..., 0] - np.sin(q64)).max(), np.abs(sincos[..., 1] - np.cos(q64)).max())


@pytest.mark.parametrize("order", ["frame", "permuted"])
@pytest.mark.parametrize("A", [1, 64, 65, 130])
def test_tree_kernels_match_the_oracle_bitwise_and_float64(A, order):
    """A = 1: one MFMA chain of fewer than 16 pairs; 64: one full block; 65 and 130: two / three blocks with a tail of 1 and of
    2 configurations (62 dead lanes that re-walk configuration A - 1 through the `scratch` branch)."""
    chain = T.tree_chain()
    leaves = R.leaf_links(R.TREE) if order == "frame" else T.permuted_leaves()
    offsets = R.visual_offsets64(R.TREE) if order == "frame" else R.visual_offsets64(R.TREE)[T.PERMUTED]
    raw = chain.joint_table(leaves)
    q = R.draw_q(R.TREE, A, 3.0, seed=A).astype(np.float32)
    out = run_kernels(raw, q, np.linalg.inv(offsets), len(leaves))
    err = sincos_error(q, out["sincos"])
    print(f"A = {A}, {order} order: sin / cos error {err:.3e} = {err * 2 ** 24:.2f} x 2^-24")
    assert err <= SINCOS_TOL
    check_against_oracle_and_float64(R.TREE, raw, leaves, offsets, q, out, f"A = {A}, {order} order")


WIDE = [0.0, -0.0, 1e-40, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 2 * np.pi, -2 * np.pi, 100.0, -100.0, 1e4, -1e4]
SLIDE = [0.0, -0.0, 0.3, -0.3]


def wide_q():
    """52 = lcm(13, 4) configurations: every revolute / continuous column cycles through WIDE (each column from another start),
    every prismatic column through SLIDE."""
    A = 52
    q = np.zeros((A, 8), np.float32)
    prismatic = R.prismatic_columns(R.TREE)
    for c in range(8):
        vals = SLIDE if c in prismatic else WIDE
        q[:, c] = np.array([vals[(a + 3 * c) % len(vals)] for a in range(A)], dtype=np.float32)
    return q


def test_sines_and_cosines_over_a_wide_range():
    """Zeros of both signs, a denormal, the multiples of pi / 2 as float32, and arguments of 100 and 10^4 radians (a continuous
    joint has no limit): the emitted sin / cos within 1e-6 of float64 sin / cos of the float32 input, the frames within 2e-6."""
    chain = T.tree_chain()
    leaves = R.leaf_links(R.TREE)
    offsets = R.visual_offsets64(R.TREE)
    raw = chain.joint_table(leaves)
    q = wide_q()
    assert q.shape == (52, 8) and np.signbit(q[q == 0]).any() and (np.abs(q) == np.float32(1e4)).any()
    assert (q == np.float32(1e-40)).any() and np.float32(1e-40) != 0
    out = run_kernels(raw, q, np.linalg.inv(offsets), len(leaves))
    rev = [c for c in range(8) if c not in R.prismatic_columns(R.TREE)]
    q64 = q.astype(np.float64)
    es = np.abs(out["sincos"][..., 0] - np.sin(q64))[:, rev]
    ec = np.abs(out["sincos"][..., 1] - np.cos(q64))[:, rev]
    big = np.abs(q[:, rev]) >= 100
    print(f"sin / cos error in units of 2^-24: sin {es.max() * 2 ** 24:.3f} cos {ec.max() * 2 ** 24:.3f} overall; "
          f"|q| >= 100: {max(es[big].max(), ec[big].max()) * 2 ** 24:.3f}; |q| < 100: {max(es[~big].max(), ec[~big].max()) * 2 ** 24:.3f}")
    assert sincos_error(q, out["sincos"]) <= SINCOS_TOL
    check_against_oracle_and_float64(R.TREE, raw, leaves, offsets, q, out, "wide q")


@pytest.mark.parametrize("A", [1, 3])
def test_static_robot_configures_with_no_joint_values(A):
    """M == 0: a null q, no sines to compute; pvamd_configure_chain returns 0 and matches the oracle bit for bit."""
    chain = T.static_chain()
    leaves = R.leaf_links(R.STATIC)
    offsets = R.visual_offsets64(R.STATIC)
    raw = chain.joint_table(leaves)
    q = np.zeros((A, 0), np.float32)
    out = run_kernels(raw, q, np.linalg.inv(offsets), len(leaves))
    check_against_oracle_and_float64(R.STATIC, raw, leaves, offsets, q, out, f"static, A = {A}")
    assert all(np.array_equal(out["stack"].reshape(2, A, 4, 4)[:, a], out["stack"].reshape(2, A, 4, 4)[:, 0]) for a in range(A))


# ---- RobotSDF on the tree robot ----
@pytest.fixture(scope="module")
def tree_robot(tmp_path_factory):
    d = tmp_path_factory.mktemp("fk_tree")
    chain = pv.build_chain_from_urdf(T.write_robot(R.TREE, d))
    robot = pv.RobotSDF(chain, path_prefix=str(d),
                        link_sdf_cls=pv.cache_link_sdf_factory(resolution=T.RES, padding=T.PADDING, device="cuda", cache_path=None))
    return robot, d


def direct_stack(robot, q):
    """The stack of a direct pvamd_configure_chain call on the table of fk_ref's leaf order; q: (A, M) float32 cuda."""
    lib = pv._lib.load()
    A, M = q.shape
    S = len(robot.sdf_to_link_name)
    raw = robot.chain.joint_table(R.leaf_links(R.TREE))
    F = len(raw) // C.sizeof(pv._lib.JointDesc)
    joints = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    scratch = torch.empty((F, 12, A), device="cuda")
    stack = torch.empty((S * A, 4, 4), device="cuda")
    pv._lib.check(lib.pvamd_configure_chain(pv._lib.ptr(joints), F, pv._lib.ptr(q), A, M, pv._lib.ptr(robot._offset_inv_dev(q.device)),
                                            S, pv._lib.ptr(None), pv._lib.ptr(scratch), pv._lib.ptr(None), pv._lib.ptr(stack),
                                            pv._lib.stream_ptr()), "pvamd_configure_chain")
    torch.cuda.synchronize()
    return stack


def test_robot_sdf_stack_on_the_tree(tree_robot):
    """Slot order, per-visual offsets and the joint column mapping at once: object_to_link_frames against stack64."""
    robot, _ = tree_robot
    assert robot.sdf_to_link_name == R.leaf_links(R.TREE) and len(robot.sdf.sdfs) == 12
    assert robot.joint_names == R.joint_names(R.TREE)
    offsets = R.visual_offsets64(R.TREE)
    off_inv = robot._offset_inv_dev(torch.device("cuda", torch.cuda.current_device())).cpu().numpy()
    assert np.abs(off_inv - np.linalg.inv(offsets)).max() < 1e-7
    q5 = R.draw_q(R.TREE, 5, 0.8, seed=5).astype(np.float32)
    q6 = R.draw_q(R.TREE, 6, 3.0, seed=6).astype(np.float32)
    for q, shape, batch in ((q5, (5, 8), (5,)), (q6, (2, 3, 8), (2, 3))):
        robot.set_joint_configuration(torch.from_numpy(q).reshape(shape))
        assert robot.configuration_batch == batch
        stack = robot.object_to_link_frames.get_matrix()
        assert stack.shape == (12 * len(q), 4, 4)
        err = np.abs(stack.cpu().numpy() - R.stack64(R.TREE, q, offsets)).max()
        print(f"RobotSDF stack against stack64, batch {batch}: {err:.3e}")
        assert err < FK_TOL
        assert torch.equal(stack, direct_stack(robot, torch.from_numpy(q).cuda()))


def test_robot_sdf_query_on_the_tree_matches_the_oracle_bitwise(tree_robot):
    robot, _ = tree_robot
    A, P = 5, 2000
    q = torch.from_numpy(R.draw_q(R.TREE, A, 0.8, seed=5).astype(np.float32))
    pts = H.uniform_points(P, [-0.6, -0.6, -0.1], [0.6, 0.6, 1.4], seed=3).cuda()
    robot.set_joint_configuration(q)
    val, grad = robot(pts)
    assert val.shape == (A, P) and grad.shape == (A, P, 3)
    stack = robot.object_to_link_frames.get_matrix().cpu().numpy()
    ogrids = [H.oracle_grid_from_cached(leaf) for leaf in robot.sdf.sdfs]
    oval, ograd, oleaf = oracle.composed_query(ogrids, stack, A, pts.cpu().numpy())
    assert np.array_equal(val.cpu().numpy(), oval, equal_nan=True)
    assert np.array_equal(grad.cpu().numpy(), ograd, equal_nan=True)
    assert len(np.unique(oleaf)) == 12 and (val < 0).any()  # every leaf wins somewhere; some points are inside the robot
    # configure_and_query_into: the same bits as set_joint_configuration followed by __call__
    v2, g2 = torch.empty((A, P), device="cuda"), torch.empty((A, P, 3), device="cuda")
    robot.configure_and_query_into(q.cuda().contiguous(), pts, v2, g2)
    assert robot.configuration_batch == (A,)
    assert torch.equal(v2, val) and torch.equal(g2.nan_to_num(7.0), grad.nan_to_num(7.0))
    assert np.array_equal(robot.object_to_link_frames.get_matrix().cpu().numpy(), stack)


def test_points_placed_by_the_float64_reference_see_their_own_leaf(tree_robot):
    """Points inside a leaf's own surface bounding box, mapped to the world by fk64 @ offset in float64: the robot's value there
    (a minimum over leaves) is at most that leaf's own cached value plus 2e-6 x the steepest |value step| / resolution between
    neighbouring voxels of that leaf's cache.  Points within 2e-6 of a voxel boundary of their own leaf may be left out (at
    most 2 %: settled on the CPU in test_fk_tree.py)."""
    robot, d = tree_robot
    q = T.probe_q()
    probes = T.probe_points(R.TREE, d, q)
    robot.set_joint_configuration(torch.from_numpy(q[0]))
    world = torch.from_numpy(np.concatenate([p["world"] for p in probes]).astype(np.float32)).cuda()
    val, _ = robot(world)
    val = val.cpu().numpy().astype(np.float64).reshape(12, T.PROBE_POINTS)
    n_excluded = 0
    for s, (p, leaf) in enumerate(zip(probes, robot.sdf.sdfs)):
        v = leaf._view
        assert v.shape == p["view"].shape and torch.equal(v.dmin, p["view"].dmin) and torch.equal(v.dres, p["view"].dres)
        grid = leaf._packed[:, 0].cpu().numpy().astype(np.float64).reshape(v.shape)
        own = grid[p["voxel"][:, 0], p["voxel"][:, 1], p["voxel"][:, 2]]
        steepest = max(np.abs(np.diff(grid, axis=ax)).max() for ax in range(3))
        slack = 2e-6 * steepest / T.RES
        keep = ~p["excluded"]
        n_excluded += int(p["excluded"].sum())
        over = (val[s] - own)[keep]
        print(f"leaf {s} ({robot.sdf_to_link_name[s]}): robot - own value max {over.max():.3e}, slack {slack:.3e}, "
              f"equal at {np.mean(over == 0):.3f} of the points")
        assert (over <= slack).all()
    assert n_excluded <= 0.02 * 12 * T.PROBE_POINTS


def test_static_robot_sdf_with_and_without_a_batch(tmp_path):
    chain = pv.build_chain_from_urdf(T.write_robot(R.STATIC, tmp_path))
    robot = pv.RobotSDF(chain, path_prefix=str(tmp_path),
                        link_sdf_cls=pv.cache_link_sdf_factory(resolution=T.RES, padding=T.PADDING, device="cuda", cache_path=None))
    assert robot.joint_names == [] and robot.sdf_to_link_name == R.leaf_links(R.STATIC)
    offsets = R.visual_offsets64(R.STATIC)
    robot.set_joint_configuration()
    assert robot.configuration_batch is None
    one = robot.object_to_link_frames.get_matrix().clone()
    assert one.shape == (2, 4, 4)
    assert np.abs(one.cpu().numpy() - R.stack64(R.STATIC, np.zeros((1, 0)), offsets)).max() < FK_TOL
    robot.set_joint_configuration(torch.zeros(3, 0))
    assert robot.configuration_batch == (3,)
    three = robot.object_to_link_frames.get_matrix().reshape(2, 3, 4, 4)
    assert all(torch.equal(three[:, a], one) for a in range(3))
    pts = H.uniform_points(500, [-0.3, -0.3, -0.2], [0.4, 0.4, 0.7], seed=1).cuda()
    val, _ = robot(pts)
    assert val.shape == (3, 500) and torch.equal(val[0], val[1]) and torch.equal(val[0], val[2])
