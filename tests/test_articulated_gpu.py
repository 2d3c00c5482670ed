"""GPU: pv.joint_normal_equations / pv.refine_joint_configuration and the four entry points of csrc/articulated.hip against
include/pvamd.h "Joint-space normal equations": the per-leaf sums bit for bit against pvamd_semantic_normal_eq on masked kinds,
the twist Jacobian and the assembly against tests/articulated_ref.py, the public results end to end, and the loop against its
pieces.  The robots are fk_ref.TREE (12 leaves, 8 joints) and fk_ref.STATIC (no joint), built as tests/test_fk_gpu.py builds them,
with nearest and with trilinear link caches."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import articulated as art
from pytorch_volumetric_amd import registration as reg
from tests import articulated_ref as AR
from tests import fk_ref as R
from tests import test_fk_tree as T
from tests.test_articulated import RECOVERY, ellipsoid_robot, recovery_case, surface_cloud
from tests.test_registration_gpu import cache_vn, transformed
from tests.test_semantic_registration_gpu import random_semantics, run_sem

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DELTA = 0.01
MODES = ("nearest", "trilinear")
FIELDS = ("cost", "gradient", "hessian", "counts", "active", "outliers", "leaf_active")


def build_robot(table, directory, mode, link_sdf_cls=None):
    chain = pv.build_chain_from_urdf(T.write_robot(table, directory))
    cls = link_sdf_cls or pv.cache_link_sdf_factory(resolution=T.RES, padding=T.PADDING, device="cuda", cache_path=None,
                                                    interpolation=mode)
    return pv.RobotSDF(chain, path_prefix=str(directory), link_sdf_cls=cls)


@pytest.fixture(scope="module")
def robots(tmp_path_factory):
    d = tmp_path_factory.mktemp("articulated_tree")
    return {mode: build_robot(R.TREE, d, mode) for mode in MODES}, d


@pytest.fixture(scope="module")
def static_robot(tmp_path_factory):
    return build_robot(R.STATIC, tmp_path_factory.mktemp("articulated_static"), "nearest")


@pytest.fixture(scope="module")
def analytic():
    return ellipsoid_robot()


def draw_q32(A, seed, scale=0.6):
    return torch.from_numpy(R.draw_q(R.TREE, A, scale, seed).astype(np.float32)).cuda()


def link_cloud(analytic, q32, n, seed, jitter=0.01):
    """n points: samples of the links' surfaces at the first configuration plus a jitter of 1 cm per axis, float32 on the device.
    Consecutive points lie on different links, so several leaves win inside one wave."""
    per = -(-n // 12)
    pts = surface_cloud(analytic, q32[0].cpu().numpy().astype(np.float64), per, seed, jitter)
    pts = pts.reshape(12, per, 3).transpose(1, 0, 2).reshape(-1, 3)[:n]
    return torch.from_numpy(pts.astype(np.float32)).cuda().contiguous()


def configure(robot, q32):
    """The float32 stack (S * A, 4, 4) of pvamd_configure_chain, into a buffer of the test's own."""
    A, M, S = q32.shape[0], len(robot.joint_names), len(robot.sdf_to_link_name)
    dev = q32.device
    return robot._configure(_lib.load(), dev, q32, A, M, S, robot._offset_inv_dev(dev))


def run_leaf_sums(robot, stack, A, pts, kinds8=None, targets=None, delta=math.inf):
    """pvamd_joint_normal_eq through ctypes: leaf_sums (A, S, 28) float64, leaf_counts (A, S, 5) int64."""
    S, N, dev = len(robot.sdf_to_link_name), pts.shape[0], pts.device
    sums = torch.empty((A, S, _lib.REG_SUMS), dtype=torch.float64, device=dev)
    counts = torch.empty((A, S, _lib.SEM_COUNTS), dtype=torch.int64, device=dev)
    scratch = _lib.scratch_buffer(_lib.joint_normal_eq_scratch_bytes(A, S, N), dev)
    mode = _lib.LEAF_MODES[robot.sdf.sdfs[0].interpolation]
    _lib.check(_lib.load().pvamd_joint_normal_eq(_lib.ptr(robot.sdf._leaf_grids(dev)), S, mode, _lib.ptr(stack), A, _lib.ptr(pts), N,
                                                 _lib.ptr(kinds8), _lib.ptr(targets), delta, _lib.ptr(sums), _lib.ptr(counts),
                                                 _lib.ptr(scratch), _lib.stream_ptr()), "pvamd_joint_normal_eq")
    return sums, counts


def run_twists(robot, q32):
    A, M, S, dev = q32.shape[0], len(robot.joint_names), len(robot.sdf_to_link_name), q32.device
    joints, F = robot._joint_table_dev(dev)
    J = torch.empty((A, S, 6, M), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().pvamd_chain_twists(_lib.ptr(joints), F, _lib.ptr(q32), A, M, _lib.ptr(robot._offset_inv_dev(dev)), S,
                                              _lib.ptr(J), _lib.stream_ptr()), "pvamd_chain_twists")
    return J


def run_assemble(leaf_sums, leaf_counts, J):
    A, S, _, M = J.shape
    sums = torch.empty((A, 1 + M + M * (M + 1) // 2), dtype=torch.float64, device=J.device)
    counts = torch.empty((A, _lib.SEM_COUNTS + S), dtype=torch.int64, device=J.device)
    _lib.check(_lib.load().pvamd_joint_assemble(_lib.ptr(leaf_sums), _lib.ptr(leaf_counts), _lib.ptr(J), A, S, M, _lib.ptr(sums),
                                                _lib.ptr(counts), _lib.stream_ptr()), "pvamd_joint_assemble")
    return sums, counts


def device_chain(robot):
    """(records, origins, axes) as the kernel is given them: the float32 origins and axes of the joint table, in float64."""
    raw = robot.chain.joint_table(robot.sdf_to_link_name)
    F = len(raw) // ctypes.sizeof(_lib.JointDesc)
    arr = (_lib.JointDesc * F).from_buffer_copy(raw)
    records = [(r.parent, r.jtype, r.jcol, r.leaf_slot) for r in arr]
    origins = np.tile(np.eye(4), (F, 1, 1))
    for f, r in enumerate(arr):
        origins[f, :3] = np.array(list(r.origin), dtype=np.float64).reshape(3, 4)
    axes = np.array([list(r.axis) for r in arr], dtype=np.float64)
    return records, origins, axes


def leaf_answers(robot, stack, A, pts):
    """Per leaf, from the existing entry points: the values of the one-leaf composition (S, A, N) float32, and of the cache's own
    query at the transformed points x (S, A, N, 3): v, n and the range decision."""
    S = len(robot.sdf_to_link_name)
    vals, xs, vs, ns, inside = [], [], [], [], []
    for s, leaf in enumerate(robot.sdf.sdfs):
        Ts = stack[s * A:(s + 1) * A].contiguous()
        one = pv.ComposedSDF([leaf], None)
        one.set_transforms(Ts, batch_dim=(A,))
        vals.append(one(pts)[0].reshape(A, -1).cpu().numpy())
        x = transformed(Ts, pts)
        v, n, ins = cache_vn(leaf, x)
        xs.append(x.cpu().numpy()), vs.append(v), ns.append(n), inside.append(ins)
    return np.stack(vals), np.stack(xs), np.stack(vs), np.stack(ns), np.stack(inside)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("mode", MODES)
def test_leaf_sums_are_the_semantic_kernel_on_masked_kinds_bit_for_bit(robots, analytic, mode):
    """Per (a, s): leaf_sums and leaf_counts[1:] of pvamd_joint_normal_eq equal pvamd_semantic_normal_eq on the pose T_s, leaf
    s's grid and the kinds replaced by IGNORE wherever s does not win; leaf_counts[0] is the in-range count of the points s
    wins.  The winner is the first minimum of the one-leaf compositions' values, and reproduces robot(points) bit for bit.  This
    pins the winner, the binning and the order of summation."""
    robot = robots[0][mode]
    S = 12
    won_everywhere, lost_somewhere = set(), False
    for N in (1, 255, 2048, 2049, 4396):
        for A in (1, 3):
            q32 = draw_q32(A, seed=100 + N + A)
            pts = link_cloud(analytic, q32, N, seed=N)
            stack = configure(robot, q32)
            vals, xs, vs, ns, inside = leaf_answers(robot, stack, A, pts)
            win = np.stack([AR.winners(vals[:, a]) for a in range(A)])
            robot.set_joint_configuration(q32)
            whole = robot(pts)[0].reshape(A, N).cpu().numpy()
            assert np.array_equal(bits(whole), bits(np.take_along_axis(vals, win[None], 0)[0])), (N, A)
            kinds, targets = random_semantics(N, seed=N + A)
            for label, kn, tg, delta in (("options", kinds, targets, DELTA), ("plain", None, None, math.inf)):
                k8 = None if kn is None else reg._prepare_semantics(kn, None, pts.device)[0]
                got_s, got_c = run_leaf_sums(robot, stack, A, pts, k8, tg, delta)
                base = torch.zeros(N, dtype=torch.uint8, device="cuda") if k8 is None else k8
                for a in range(A):
                    for s in range(S):
                        mine = torch.from_numpy(win[a] == s).cuda()
                        masked = torch.where(mine, base, torch.full_like(base, pv.POINT_IGNORE))
                        want_s, want_c = run_sem(robot.sdf.sdfs[s], stack[s * A + a].reshape(1, 4, 4).contiguous(), pts, masked, tg,
                                                 delta)
                        assert torch.equal(got_s[a, s].view(torch.int64), want_s[0].view(torch.int64)), (label, N, A, a, s)
                        assert torch.equal(got_c[a, s, 1:], want_c[0, 1:]), (label, N, A, a, s)
                        assert int(got_c[a, s, 0]) == int((inside[s, a] & (win[a] == s)).sum()), (label, N, A, a, s)
                        if not mine.any():
                            assert (got_s[a, s] == 0).all() and not torch.signbit(got_s[a, s]).any()
            for a in range(A):
                leaves = set(win[a].tolist())
                won_everywhere |= leaves
                lost_somewhere |= len(leaves) < S
    assert won_everywhere == set(range(S)) and lost_somewhere


def test_sixty_four_leaves_fill_the_mask(robots):
    """The most leaves the kernel takes: the twelve link caches repeated to 64 leaves on a 4 x 4 x 4 lattice 0.3 m apart, points
    around every lattice site in an order that mixes the leaves inside a wave.  Every leaf wins, the last one (bit 63 of the
    wave's mask of leaves) included, and every (a, s) equals pvamd_semantic_normal_eq on the masked kinds bit for bit."""
    robot = robots[0]["nearest"]
    S, A, per = _lib.JOINT_MAX_LEAVES, 2, 40
    leaves = [robot.sdf.sdfs[i % 12] for i in range(S)]
    grids = pv.ComposedSDF(leaves, None)._leaf_grids(torch.device("cuda", torch.cuda.current_device()))
    rng = np.random.default_rng(17)
    sites = np.array([[i // 16, (i // 4) % 4, i % 4] for i in range(S)], dtype=np.float64) * 0.3
    stack = torch.eye(4).repeat(S * A, 1, 1)
    for s in range(S):
        for a in range(A):
            stack[s * A + a, :3, 3] = torch.from_numpy(-sites[s] + 0.004 * a)  # leaf s sits at its site
    stack = stack.cuda().contiguous()
    pts = (sites[None] + rng.uniform(-0.05, 0.05, (per, S, 3))).reshape(-1, 3)  # consecutive points belong to different leaves
    pts = torch.from_numpy(pts.astype(np.float32)).cuda().contiguous()
    N = pts.shape[0]
    assert N > _lib.REG_CHUNK
    kinds, targets = random_semantics(N, seed=18)
    k8 = reg._prepare_semantics(kinds, None, pts.device)[0]
    sums = torch.empty((A, S, _lib.REG_SUMS), dtype=torch.float64, device="cuda")
    counts = torch.empty((A, S, _lib.SEM_COUNTS), dtype=torch.int64, device="cuda")
    scratch = _lib.scratch_buffer(_lib.joint_normal_eq_scratch_bytes(A, S, N), "cuda")
    _lib.check(_lib.load().pvamd_joint_normal_eq(_lib.ptr(grids), S, _lib.LEAF_MODES["nearest"], _lib.ptr(stack), A, _lib.ptr(pts), N,
                                                 _lib.ptr(k8), _lib.ptr(targets), DELTA, _lib.ptr(sums), _lib.ptr(counts),
                                                 _lib.ptr(scratch), _lib.stream_ptr()), "pvamd_joint_normal_eq")
    vals = np.stack([cache_vn(leaves[s], transformed(stack[s * A:(s + 1) * A].contiguous(), pts))[0] for s in range(S)])
    for a in range(A):
        win = AR.winners(vals[:, a])
        assert set(win.tolist()) == set(range(S))
        for s in range(S):
            masked = torch.where(torch.from_numpy(win == s).cuda(), k8, torch.full_like(k8, pv.POINT_IGNORE))
            want_s, want_c = run_sem(leaves[s], stack[s * A + a].reshape(1, 4, 4).contiguous(), pts, masked, targets, DELTA)
            assert torch.equal(sums[a, s].view(torch.int64), want_s[0].view(torch.int64)), (a, s)
            assert torch.equal(counts[a, s, 1:], want_c[0, 1:]), (a, s)
    assert int(counts[:, :, 1:4].sum()) > 0


def test_chain_twists_against_the_reference(robots):
    """pvamd_chain_twists against articulated_ref on the joint table's own float32 origins and axes, at the float32 q.  Per entry
    |difference| <= 64 F 2^-52 max(1, reach): a float64 chain of at most F compositions, each entry a few roundings relative to
    the reach, with device sin / cos a few ulp from numpy's."""
    robot = robots[0]["nearest"]
    records, origins, axes = device_chain(robot)
    assert records == R.expected_records(R.TREE) and len(records) == 15
    F, reach = len(records), AR.reach(records, origins)
    offset_inv = robot._offset_inv_dev(torch.device("cuda", torch.cuda.current_device())).cpu().numpy().astype(np.float64)
    worst = 0.0
    for A, scale, seed in ((1, 0.6, 1), (3, 0.8, 2), (70, 3.0, 3)):
        q32 = draw_q32(A, seed, scale)
        J = run_twists(robot, q32).cpu().numpy()
        _, want = AR.stack_and_twists(records, origins, axes, q32.cpu().numpy().astype(np.float64), offset_inv)
        bound = 64 * F * EPS * max(1.0, reach)
        err = float(np.abs(J - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (A, err, bound)
        for s in range(12):
            others = [k for k in range(8) if k not in AR.ancestors(records, s)]
            assert (J[:, s][:, :, others] == 0.0).all()
    print(f"pvamd_chain_twists against the reference: worst error / bound = {worst:.3g} (reach {reach:.3g}, F {F})")


@pytest.mark.parametrize("mode", MODES)
def test_assembly_against_numpy_on_the_kernels_own_sums(robots, analytic, mode):
    """pvamd_joint_assemble against math.fsum of the products J[r][i] H6[r][c] J[c][j] of the GPU's own leaf sums and J.  Per entry
    |difference| <= (36 S + 8) 2^-53 (|J|^T |H6| |J|) (and the like for the gradient and the cost): at most 6 S + 6 roundings on the
    device and two per product in the reference."""
    robot = robots[0][mode]
    A, N, S, M = 3, 2049, 12, 8
    q32 = draw_q32(A, seed=31)
    pts = link_cloud(analytic, q32, N, seed=32)
    kinds, targets = random_semantics(N, seed=33)
    k8 = reg._prepare_semantics(kinds, None, pts.device)[0]
    leaf_sums, leaf_counts = run_leaf_sums(robot, configure(robot, q32), A, pts, k8, targets, DELTA)
    J = run_twists(robot, q32)
    sums, counts = run_assemble(leaf_sums, leaf_counts, J)
    Ls, Jn, got, lc = leaf_sums.cpu().numpy(), J.cpu().numpy(), sums.cpu().numpy(), leaf_counts.cpu().numpy()
    k = (36 * S + 8) * EPS / 2
    worst = 0.0
    for a in range(A):
        parts = [AR.unpack6(Ls[a, s]) for s in range(S)]
        c6 = np.array([p[0] for p in parts])
        g6 = np.stack([p[1] for p in parts])
        H6 = np.stack([p[2] for p in parts])
        want = [math.fsum(c6)] + [math.fsum((Jn[a, :, :, i] * g6).ravel()) for i in range(M)]
        mag = [math.fsum(np.abs(c6))] + [math.fsum(np.abs(Jn[a, :, :, i] * g6).ravel()) for i in range(M)]
        for i in range(M):
            for j in range(i, M):
                t = Jn[a, :, :, None, i] * H6 * Jn[a, :, None, :, j]
                want.append(math.fsum(t.ravel()))
                mag.append(math.fsum(np.abs(t).ravel()))
        err, bound = np.abs(got[a] - np.array(want)), k * np.array(mag)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (a, err, bound)
        assert np.array_equal(counts[a, :5].cpu().numpy(), lc[a].sum(0))
        assert np.array_equal(counts[a, 5:].cpu().numpy(), lc[a, :, 1:4].sum(-1))
    print(f"pvamd_joint_assemble against fsum [{mode}]: worst error / bound = {worst:.3g}")
    ne = pv.joint_normal_equations(robot, q32, pts, semantics=kinds, targets=targets, huber_delta=DELTA)
    assert torch.equal(ne.hessian, ne.hessian.transpose(1, 2))
    kk = 1000. * 1000. / N
    assert torch.equal(ne.cost, sums[:, 0] * kk) and torch.equal(ne.gradient, sums[:, 1:1 + M] * kk)


def contract_reference(robot, q32, pts, kinds, targets, delta):
    """The contract end to end, in float64 from the existing entry points' answers: per configuration the winner, its x, (v, n)
    and range decision, the per-pair terms, their per-leaf fsum and magnitudes, assembled with the device's own J (checked on
    its own above)."""
    A = q32.shape[0]
    stack = configure(robot, q32)
    vals, xs, vs, ns, inside = leaf_answers(robot, stack, A, pts)
    J = run_twists(robot, q32).cpu().numpy() if len(robot.joint_names) else np.zeros((A, vals.shape[0], 6, 0))
    S, N = vals.shape[0], pts.shape[0]
    idx = np.arange(N)
    out = []
    for a in range(A):
        win = AR.winners(vals[:, a])
        terms, flags, _, _, _ = AR.pair_terms(vs[win, a, idx], ns[win, a, idx], xs[win, a, idx], kinds, targets, delta)
        sums = np.stack([AR.fsum_columns(terms[win == s]) for s in range(S)])
        mags = np.stack([AR.fsum_columns(np.abs(terms[win == s])) for s in range(S)])
        out.append(dict(value=AR.assemble(sums, J[a]), mag=AR.assemble_magnitude(mags, J[a]),
                        counts=int(inside[win, a, idx].sum()), active=flags[:, :3].sum(0), outliers=int(flags[:, 3].sum()),
                        leaf_active=np.array([flags[win == s, :3].sum() for s in range(S)]), nan=bool(np.isnan(sums).any())))
    return out


def check_public(ne, ref, N, S, scale, label):
    k = scale * scale / N
    worst = 0.0
    for a, e in enumerate(ref):
        assert int(ne.counts[a]) == e["counts"] and ne.active[a].tolist() == e["active"].tolist(), (label, a)
        assert int(ne.outliers[a]) == e["outliers"] and ne.leaf_active[a].tolist() == e["leaf_active"].tolist(), (label, a)
        assert not e["nan"]
        for got, want, mag in zip((ne.cost[a], ne.gradient[a], ne.hessian[a]), e["value"], e["mag"]):
            err = np.abs(got.cpu().numpy() / k - np.asarray(want))
            bound = (N + 36 * S + 64) * EPS * np.asarray(mag)
            if err.size:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (label, a, err, bound)
    return worst


@pytest.mark.parametrize("mode", MODES)
def test_public_results_against_the_contract(robots, analytic, static_robot, mode):
    robot = robots[0][mode]
    worst = 0.0
    for N, A in ((255, 1), (2049, 3), (4396, 2)):
        q32 = draw_q32(A, seed=40 + N)
        pts = link_cloud(analytic, q32, N, seed=41 + N)
        kinds, targets = random_semantics(N, seed=42 + N)
        for label, kw in (("options", dict(semantics=kinds, targets=targets, huber_delta=DELTA)), ("plain", {})):
            ne = pv.joint_normal_equations(robot, q32, pts, scale=10., **kw)
            assert ne.cost.shape == (A,) and ne.gradient.shape == (A, 8) and ne.hessian.shape == (A, 8, 8)
            assert ne.leaf_active.shape == (A, 12) and ne.active.shape == (A, 3)
            assert all(t.dtype == torch.float64 for t in ne[:3]) and all(t.dtype == torch.int64 for t in ne[3:])
            assert torch.equal(ne.hessian, ne.hessian.transpose(1, 2)) and not any(t.requires_grad for t in ne)
            ref = contract_reference(robot, q32, pts, kinds.cpu().numpy() if kw else None, targets.cpu().numpy() if kw else None,
                                     DELTA if kw else math.inf)
            worst = max(worst, check_public(ne, ref, N, 12, 10., (label, N, A)))
            assert torch.equal(ne.leaf_active.sum(-1), ne.active.sum(-1))
    print(f"public results against the contract [{mode}]: worst error / bound = {worst:.3g}")
    if mode == "nearest":
        # a (M,) configuration, leading dimensions of the points, and the robot without joints
        q1 = draw_q32(1, seed=50)[0]
        pts = link_cloud(analytic, q1[None], 600, seed=51)
        a = pv.joint_normal_equations(robot, q1, pts.reshape(2, 300, 3))
        b = pv.joint_normal_equations(robot, q1[None], pts)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and a.cost.shape == (1,)
        spts = torch.from_numpy(np.random.default_rng(5).uniform(-0.1, 0.4, (700, 3)).astype(np.float32)).cuda()
        for qs in (torch.zeros((3, 0)), torch.zeros(0)):
            ne = pv.joint_normal_equations(static_robot, qs, spts)
            A = 3 if qs.dim() == 2 else 1
            assert ne.gradient.shape == (A, 0) and ne.hessian.shape == (A, 0, 0) and ne.leaf_active.shape == (A, 2)
            ref = contract_reference(static_robot, torch.zeros((A, 0), device="cuda"), spts, None, None, math.inf)
            check_public(ne, ref, 700, 2, 1000., "static")
        res = pv.refine_joint_configuration(static_robot, torch.zeros((3, 0)), spts, iterations=4)
        assert res.joint_config.shape == (3, 0) and torch.equal(res.cost, res.initial_cost) and (res.accepted == 1).all()
        assert torch.equal(res.cost, pv.joint_normal_equations(static_robot, torch.zeros((3, 0)), spts).cost)
        empty = pv.joint_normal_equations(robot, torch.zeros((0, 8)), pts)
        assert empty.cost.shape == (0,) and empty.hessian.shape == (0, 8, 8) and empty.leaf_active.shape == (0, 12)
        assert pv.refine_joint_configuration(robot, torch.zeros((0, 8)), pts).joint_config.shape == (0, 8)


@pytest.mark.parametrize("mode", MODES)
def test_a_nan_record_touches_only_the_configurations_that_read_it(robots, analytic, mode):
    """A NaN record in the head's cache, and a point that reads it in configurations 0 and 2; in configuration 1 the head is
    turned by 1 rad and the point reads records four voxels away."""
    robot = robots[0][mode]
    s = 11
    leaf = robot.sdf.sdfs[s]
    assert robot.sdf_to_link_name[s] == "head"
    view = leaf._view
    dmin, dres = np.array([float(t) for t in view.dmin]), np.array([float(t) for t in view.dres])
    ijk = np.rint((np.array([0.07, 0.01, 0.03]) - dmin) / dres).astype(np.int64)
    assert (ijk >= 2).all() and (ijk < np.array(tuple(view.shape)) - 2).all()
    centre = dmin + ijk * dres
    k = int(np.ravel_multi_index(tuple(ijk), tuple(view.shape)))
    q32 = draw_q32(1, seed=60).repeat(3, 1)
    q32[1, 7] += 1.0  # j_head
    stack = configure(robot, q32)
    to_object = AR.rigid_inverse(stack[s * 3].cpu().numpy().astype(np.float64))
    p = torch.from_numpy((to_object[:3, :3] @ centre + to_object[:3, 3]).astype(np.float32)).cuda()
    pts = torch.cat((link_cloud(analytic, q32, 500, seed=61, jitter=0.0), p[None])).contiguous()
    moved = transformed(stack[s * 3:s * 3 + 3].contiguous(), p[None]).cpu().numpy()[:, 0]
    assert np.abs(moved[0] - centre).max() < 1e-5 and np.abs(moved[1] - centre).max() > 3 * dres.max()
    clean = pv.joint_normal_equations(robot, q32, pts)
    old = leaf._packed[k].clone()
    try:
        leaf._packed[k] = math.nan  # the whole record: value and gradient
        assert torch.isnan(leaf(torch.from_numpy(centre.astype(np.float32)).cuda()[None])[0]).all()
        ne = pv.joint_normal_equations(robot, q32, pts)
        res = pv.refine_joint_configuration(robot, q32, pts, iterations=2)
    finally:
        leaf._packed[k] = old
    for a in (0, 2):
        assert torch.isnan(ne.cost[a]) and torch.isnan(ne.gradient[a]).all() and torch.isnan(ne.hessian[a]).all()
        assert torch.equal(res.joint_config[a], q32[a]) and torch.isnan(res.cost[a]) and int(res.accepted[a]) == 1
    for f in ("cost", "gradient", "hessian"):
        assert torch.equal(getattr(ne, f)[1], getattr(clean, f)[1]), f
    assert not torch.isnan(res.cost[1]) and res.cost[1] <= res.initial_cost[1]
    again = pv.joint_normal_equations(robot, q32, pts)
    assert all(torch.equal(x, y) for x, y in zip(again, clean))  # the record is back


@pytest.mark.parametrize("mode", MODES)
def test_two_calls_and_a_graph_replay_give_the_same_bits_and_the_robot_stays(robots, analytic, mode):
    robot = robots[0][mode]
    A, N = 5, 3 * _lib.REG_CHUNK + 17
    q32 = draw_q32(A, seed=70)
    pts = link_cloud(analytic, q32, N, seed=71)
    kinds, targets = random_semantics(N, seed=72)
    kw = dict(semantics=kinds, targets=targets, huber_delta=DELTA)
    # the robot's own configuration: another one, read before and after
    mine = draw_q32(2, seed=73)
    robot.set_joint_configuration(mine)
    before_q, before_v, before_g = robot.q, *robot(pts)
    before_tf = robot.sdf._tf_matrix.clone()
    a = pv.joint_normal_equations(robot, q32, pts, **kw)
    b = pv.joint_normal_equations(robot, q32, pts, **kw)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    ra = pv.refine_joint_configuration(robot, q32, pts, iterations=3, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gn = pv.joint_normal_equations(robot, q32, pts, **kw)
        gr = pv.refine_joint_configuration(robot, q32, pts, iterations=3, **kw)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for f in FIELDS:
            assert torch.equal(getattr(a, f), getattr(gn, f)), f
        for f in ("joint_config", "cost", "initial_cost", "accepted"):
            assert torch.equal(getattr(ra, f), getattr(gr, f)), f
    assert robot.q is before_q and torch.equal(robot.q, mine) and torch.equal(robot.sdf._tf_matrix, before_tf)
    after_v, after_g = robot(pts)
    assert torch.equal(after_v, before_v) and torch.equal(after_g, before_g)
    assert (ra.cost <= ra.initial_cost).all() and (ra.accepted >= 1).all() and ra.joint_config.dtype == torch.float32


def test_step_at_the_joint_limit_of_the_kernel():
    """pvamd_joint_lm_step alone at M = PVAMD_JOINT_MAX = 32 (every lane of the factorisation busy) and at M = 5, on synthetic
    sums: a well-conditioned system, then a rejected evaluation, then an indefinite matrix (failed pivot: zero step, q_acc
    copied, lambda raised), with limits.  Decisions and lambda equal articulated_ref.lm_step's; q_try within its bound."""
    lib = _lib.load()
    rng = np.random.default_rng(23)
    for M in (_lib.JOINT_MAX, 5):
        A, P = 3, 1 + M + M * (M + 1) // 2
        iu = np.triu_indices(M)
        lim = np.stack((np.full(M, -0.5), np.full(M, 0.5)), axis=-1)
        lim_d = torch.from_numpy(lim).cuda()
        q0 = rng.uniform(-0.3, 0.3, (A, M))
        states = [AR.JointState(q_try=q0[a].copy(), lam=1e-3) for a in range(A)]
        q_try = torch.from_numpy(q0).cuda()
        q_acc, sums_acc = torch.empty_like(q_try), torch.empty((A, P), dtype=torch.float64, device="cuda")
        lam = torch.full((A,), 1e-3, dtype=torch.float64, device="cuda")
        accepted = torch.zeros((A,), dtype=torch.int32, device="cuda")
        q_next = torch.empty((A, M), dtype=torch.float32, device="cuda")
        for it, kind in enumerate(("spd", "worse", "indefinite", "spd")):
            rows, parts = np.zeros((A, P)), []
            for a in range(A):
                B = rng.standard_normal((M + 3, M))
                H = B.T @ B + np.eye(M)
                if kind == "indefinite":
                    H[0, 0] = -1.0
                if a == 2:
                    H[1, :] = H[:, 1] = 0.0  # a joint nothing observes
                g = rng.standard_normal(M)
                g[1] = 0.0 if a == 2 else g[1]
                cost = {"spd": 10.0 - 2 * it, "worse": 11.0, "indefinite": 5.0}[kind]  # 10, 11 (rejected), 5, 4
                rows[a] = np.concatenate(([cost], g, H[iu]))
                parts.append((cost, g, H))
            sums = torch.from_numpy(rows).cuda()
            _lib.check(lib.pvamd_joint_lm_step(A, M, _lib.ptr(sums), int(it == 0), _lib.ptr(q_acc), _lib.ptr(sums_acc), _lib.ptr(lam),
                                               _lib.ptr(accepted), _lib.ptr(q_try), _lib.ptr(q_next), _lib.ptr(lim_d), 10.0, 0.1,
                                               reg.LAMBDA_MIN, reg.LAMBDA_MAX, _lib.stream_ptr()), "pvamd_joint_lm_step")
            for a, st in enumerate(states):
                before = st.bound
                AR.lm_step(st, *parts[a], it == 0, limits=lim)
                assert int(accepted[a]) == st.accepted and float(lam[a]) == st.lam, (M, kind, a)
                assert np.array_equal(q_acc[a].cpu().numpy(), st.q_acc), (M, kind, a)  # copies of values both sides hold exactly
                err = np.abs(q_try[a].cpu().numpy() - st.q_try).max()
                assert err <= st.bound - before, (M, kind, a, err)
                assert np.array_equal(q_next[a].cpu().numpy(), q_try[a].cpu().numpy().astype(np.float32))
                assert np.array_equal(sums_acc[a].cpu().numpy()[0], st.cost_acc)
                if kind == "indefinite":
                    assert np.array_equal(q_try[a].cpu().numpy(), st.q_acc) and not st.dq.any()
                if a == 2:
                    assert q_try[a, 1].item() == st.q_acc[1]  # the unobserved joint does not move
                assert (q_try[a] >= -0.5).all() and (q_try[a] <= 0.5).all()
            # both loops go on from the device's trial values
            for a, st in enumerate(states):
                st.q_try = q_try[a].cpu().numpy().copy()
        assert [st.accepted for st in states] == [3, 3, 3]


def hand_loop(robot, q0, pts, iterations, limits=None, **kw):
    """refine_joint_configuration's loop by hand: pv.joint_normal_equations at the float32 trial values, then the numpy step.
    (The step does not depend on the scale: it is the same factor on both sides of its equation and of its comparison.)"""
    def evaluate(q32):
        ne = pv.joint_normal_equations(robot, torch.from_numpy(q32).cuda(), pts, **kw)
        return ne.cost.cpu().numpy(), ne.gradient.cpu().numpy(), ne.hessian.cpu().numpy()
    return AR.refine(evaluate, q0, iterations=iterations, limits=limits)


@pytest.mark.parametrize("mode", MODES)
def test_the_loop_is_the_pieces(robots, analytic, mode):
    """refine_joint_configuration against a hand loop over joint_normal_equations and articulated_ref's step, after every number
    of iterations up to four.  The decisions (accepted) are equal.  The joint values, asked for in float64 so that nothing is
    rounded on the way out, agree within the rounding of the steps taken so far (articulated_ref.lm_step states the bound of one
    step; the float32 trial values of both loops are then the same, so the sums they are given are the same bits).  Also with
    limits that bind one revolute and one prismatic joint: no returned value lies outside them."""
    robot = robots[0][mode]
    q_true, start = recovery_case()
    pts = torch.from_numpy(surface_cloud(analytic, q_true[0], 40, seed=80, jitter=0.002).astype(np.float32)).cuda()
    kinds, targets = random_semantics(pts.shape[0], seed=81)
    kinds[kinds == pv.POINT_IGNORE] = pv.POINT_SURFACE
    targets = targets * 0.1
    M, ITS = 8, 4
    lim = np.array([[-10.0, 10.0]] * M)
    lim[1] = [start[0, 1] - 0.004, start[0, 1] + 0.004]    # j_shoulder, revolute
    lim[4] = [start[0, 4] - 0.0004, start[0, 4] + 0.0004]  # j_finger_a, prismatic
    lim32 = art._check_limits(torch.from_numpy(lim), M)
    start64 = torch.from_numpy(start.astype(np.float64))
    for label, kw, limits in (("plain", {}, None), ("options", dict(semantics=kinds, targets=targets, huber_delta=DELTA), None),
                              ("limits", {}, lim)):
        states, initial = hand_loop(robot, start, pts, ITS, limits=None if limits is None else lim32, **kw)
        worst = 0.0
        for it in range(1, ITS + 1):
            res = pv.refine_joint_configuration(robot, start64, pts, iterations=it,
                                                joint_limits=None if limits is None else torch.from_numpy(limits), **kw)
            assert res.joint_config.dtype == torch.float64 and res.joint_config.device.type == "cpu"
            assert np.array_equal(res.initial_cost.cpu().numpy(), initial), label
            got = res.joint_config.numpy()
            assert res.accepted.tolist() == [st.history[it][1] for st in states], (label, it)
            for a, st in enumerate(states):
                want, _, bound = st.history[it]
                err = float(np.abs(got[a] - want).max())
                worst = max(worst, err / max(bound, 1e-300))
                assert err <= bound, (label, it, a, err, bound)
            if limits is not None:
                assert (got >= lim[:, 0]).all() and (got <= lim[:, 1]).all(), (label, it)
        assert (res.cost <= res.initial_cost).all() and max(st.accepted for st in states) >= 2
        print(f"the loop is the pieces [{mode}, {label}]: worst |q - q_hand| / bound = {worst:.3g}, accepted {res.accepted.tolist()}")
        if limits is not None:
            assert (np.isin(got[:, 1], lim32[1]) | np.isin(got[:, 4], lim32[4])).any(), "no limit was binding"
            r32 = pv.refine_joint_configuration(robot, torch.from_numpy(start), pts, iterations=ITS, joint_limits=torch.from_numpy(limits))
            o32 = r32.joint_config.numpy().astype(np.float64)
            assert r32.joint_config.dtype == torch.float32 and (o32 >= lim[:, 0]).all() and (o32 <= lim[:, 1]).all()


@pytest.mark.parametrize("mode", MODES)
def test_recovery_on_caches(robots, analytic, mode):
    """tests/test_articulated.py's scenario on the link caches: every configuration accepts at least twice and ends below its
    start.  Printed, not asserted: how far from q_true it starts and ends."""
    robot = robots[0][mode]
    q_true, start = recovery_case()
    pts = torch.from_numpy(surface_cloud(analytic, q_true[0], RECOVERY["per_leaf"], RECOVERY["cloud_seed"]).astype(np.float32)).cuda()
    res = pv.refine_joint_configuration(robot, torch.from_numpy(start).cuda(), pts, iterations=RECOVERY["iterations"])
    before = np.abs(start.astype(np.float64) - q_true).max(axis=1)
    after = np.abs(res.joint_config.cpu().numpy().astype(np.float64) - q_true).max(axis=1)
    print(f"recovery on caches [{mode}]: accepted {res.accepted.tolist()}, cost {res.initial_cost.tolist()} -> {res.cost.tolist()}, "
          f"|q - q_true|_inf {before.tolist()} -> {after.tolist()}")
    assert res.joint_config.is_cuda and (res.accepted >= 2).all() and (res.cost < res.initial_cost).all()


def test_refusals(robots, tmp_path):
    (by_mode, directory), q, cloud = robots, torch.zeros(8), torch.zeros((5, 3), device="cuda")
    with pytest.raises(ValueError, match="leaf 0"):
        pv.joint_normal_equations(build_robot(R.TREE, directory, None, link_sdf_cls=pv.MeshSDF), q, cloud)
    mixed = build_robot(R.TREE, directory, "nearest")
    mixed.sdf.sdfs[3].interpolation = "trilinear"
    for call in (pv.joint_normal_equations, pv.refine_joint_configuration):
        with pytest.raises(ValueError, match="one interpolation"):
            call(mixed, q, cloud)

    class Foreign:
        def __init__(self, chain):
            self._chain = chain

        def __getattr__(self, name):
            return getattr(self._chain, name)

    foreign = build_robot(R.TREE, directory, "nearest")
    foreign.chain = Foreign(foreign.chain)
    for call in (pv.joint_normal_equations, pv.refine_joint_configuration):
        with pytest.raises(ValueError, match="kinematics.Chain"):
            call(foreign, q, cloud)


def test_peak_memory_has_no_per_pair_buffer(robots, analytic):
    """Above the inputs, a call at A = 64, N = 16,384 allocates its slab (264 A S chunks bytes), its stack, leaf sums, J and
    outputs, and the converted kinds (one byte a point, through int64 temporaries of N elements): less than one (A, N) float32
    buffer."""
    robot = robots[0]["trilinear"]
    A, N, S, M = 64, 16384, 12, 8
    q32 = draw_q32(A, seed=90)
    pts = link_cloud(analytic, q32, N, seed=91)
    kinds, targets = random_semantics(N, seed=92)
    kw = dict(semantics=kinds, targets=targets, huber_delta=DELTA)
    pv.joint_normal_equations(robot, q32[:2], pts[:10], semantics=kinds[:10], targets=targets[:10], huber_delta=DELTA)
    pv.joint_normal_equations(robot, q32, pts[:10], semantics=kinds[:10], targets=targets[:10], huber_delta=DELTA)  # per-A scratch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ne = pv.joint_normal_equations(robot, q32, pts, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    slab = _lib.joint_normal_eq_scratch_bytes(A, S, N)
    assert slab == 264 * A * S * 8
    P = 1 + M + M * (M + 1) // 2
    small = A * S * (64 + 28 * 8 + 5 * 8 + 6 * M * 8) + 3 * A * (P + M * M) * 8 + 2 * A * (5 + S) * 8
    allowed = slab + small + 4 * 8 * N + (1 << 20)
    print(f"peak extra memory {peak} B, allowed {allowed} B (slab {slab} B); one (A, N) float32 buffer would be {4 * A * N} B")
    assert peak <= allowed, (peak, allowed)
    assert 4 * A * N > allowed
    assert (ne.counts <= N).all()
