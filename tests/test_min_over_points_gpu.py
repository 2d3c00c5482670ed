"""-m gpu: ComposedSDF / RobotSDF.min_over_points (csrc/min_over_points.hip) against the contract of include/pvamd.h "Minimum over
points": the composed query (per leaf: one-leaf compositions) reduced with the index rule restated here, bit for bit; the
nearest float32 answers also against the C oracle, the trilinear float32 ones against tests/interp_ref.c; edge cases, the
generic path, reproducibility, autograd against autograd through __call__ gathered at the indices, peak memory, graph capture."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from oracle import oracle
from tests import helpers as H
from tests.test_interp_gpu import build_robot, composed_ref_f32

pytestmark = pytest.mark.gpu


def restated_argmin(v):
    """(A, P) host array -> (A,) indices: the first NaN if the row holds one, else the first index whose value equals the row's
    minimum (-0.0 == +0.0)."""
    v = np.asarray(v)
    out = np.empty(v.shape[0], np.int64)
    for a in range(v.shape[0]):
        nan = np.isnan(v[a])
        out[a] = int(np.argmax(nan)) if nan.any() else int(np.argmax(v[a] == v[a].min()))
    return out


def same_bits(a, b):
    """Equal bit patterns, NaNs compared as NaN (payloads aside)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    it = np.int32 if a.dtype == np.float32 else np.int64
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(it), b[~nb].view(it)))


def batch_of(comp):
    return tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()


def one_leaf(comp, s):
    one = pv.ComposedSDF([comp.sdfs[s]], None)
    one.set_transforms(comp._tf_matrix.detach()[comp.ith_transform_slice(s)], batch_dim=comp.tsf_batch)
    return one


def expected(comp, pts, per_leaf):
    """(values, indices, gradients) as host arrays from __call__ + the restated rule."""
    with torch.no_grad():
        if per_leaf:
            parts = [expected(one_leaf(comp, s), pts, False) for s in range(len(comp.sdfs))]
            nb = len(batch_of(comp))
            return tuple(np.stack(t, axis=nb) for t in zip(*parts))
        v, g = comp(pts)
    batch = batch_of(comp)
    A = math.prod(batch)
    v = v.reshape(A, -1).cpu().numpy()
    g = g.reshape(A, -1, 3).cpu().numpy()
    idx = restated_argmin(v)
    rows = np.arange(A)
    return v[rows, idx].reshape(batch), idx.reshape(batch), g[rows, idx].reshape(*batch, 3)


def check(comp, pts, per_leaf, exp=None):
    res = comp.min_over_points(pts, per_leaf=per_leaf)
    assert isinstance(res, pv.MinOverPoints)
    ev, ei, eg = exp if exp is not None else expected(comp, pts, per_leaf)
    assert res.indices.dtype == torch.int64
    assert np.array_equal(res.indices.cpu().numpy(), ei)
    assert same_bits(res.values.cpu().numpy(), ev), "values"
    assert same_bits(res.gradients.cpu().numpy(), eg), "gradients"
    return res


# ---------------------------------------------------------------- compositions
@pytest.fixture(scope="module")
def cache():
    return W.build_c2_cache()


@pytest.fixture(scope="module")
def cache_tri():
    c = W.build_c2_cache()
    c.interpolation = "trilinear"
    return c


@pytest.fixture(scope="module")
def robot():
    return W.build_c4()


@pytest.fixture(scope="module")
def robot_tri():
    return build_robot(interpolation="trilinear")


def c3(leaf, A=3, seed=0):
    comp = pv.ComposedSDF([leaf] * 8, None)
    comp.set_transforms(W.random_rigid(8 * A, seed=seed, trans=0.2).cuda(), batch_dim=(A,))
    return comp


def c3_pts(n, seed):
    return W.c3_points(n, seed=seed)


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("per_leaf", [False, True], ids=["overall", "per_leaf"])
def test_c3_and_c4_bit_exact(cache, cache_tri, robot, robot_tri, tri, dtype, per_leaf):
    comp = c3(cache_tri if tri else cache)
    check(comp, c3_pts(50_000, seed=1).to(dtype), per_leaf)
    r = robot_tri if tri else robot
    r.set_joint_configuration(W.c4_joint_configs(16, seed=3).cuda())
    pts = W.c4_points(40_000, seed=5).to(dtype)
    res = check(r.sdf, pts, per_leaf)
    # the robot method is the composition's
    rr = r.min_over_points(pts, per_leaf=per_leaf)
    assert torch.equal(rr.indices, res.indices) and torch.equal(rr.values, res.values)
    S = len(r.sdf_to_link_name)
    assert res.values.shape == ((16, S) if per_leaf else (16,)) and res.values.dtype == dtype
    assert res.gradients.shape == res.values.shape + (3,)


def test_nearest_against_oracle(cache, robot):
    robot.set_joint_configuration(W.c4_joint_configs(6, seed=11).cuda())
    pts = W.c4_points(30_000, seed=12)
    comp = robot.sdf
    grids = [H.oracle_grid_from_cached(c) for c in comp.sdfs]
    tfm = comp._tf_matrix.detach().cpu().numpy()
    ov, og, _ = oracle.composed_query(grids, tfm, 6, pts.cpu().numpy())
    idx = restated_argmin(ov)
    res = comp.min_over_points(pts)
    assert np.array_equal(res.indices.cpu().numpy(), idx)
    assert same_bits(res.values.cpu().numpy(), ov[np.arange(6), idx])
    assert same_bits(res.gradients.cpu().numpy(), og[np.arange(6), idx])
    # per leaf: the oracle over one leaf at a time
    resl = comp.min_over_points(pts, per_leaf=True)
    S = len(comp.sdfs)
    for s in range(S):
        v, g, _ = oracle.composed_query([grids[s]], tfm[s * 6:(s + 1) * 6], 6, pts.cpu().numpy())
        i = restated_argmin(v)
        assert np.array_equal(resl.indices[:, s].cpu().numpy(), i)
        assert same_bits(resl.values[:, s].cpu().numpy(), v[np.arange(6), i])
        assert same_bits(resl.gradients[:, s].cpu().numpy(), g[np.arange(6), i])


def test_trilinear_against_interp_ref(robot_tri):
    robot_tri.set_joint_configuration(W.c4_joint_configs(5, seed=13).cuda())
    pts = W.c4_points(30_000, seed=14)
    comp = robot_tri.sdf
    rv, rg, _ = composed_ref_f32(comp.sdfs, comp._tf_matrix, pts)
    idx = restated_argmin(rv)
    res = comp.min_over_points(pts)
    assert np.array_equal(res.indices.cpu().numpy(), idx)
    assert same_bits(res.values.cpu().numpy(), rv[np.arange(5), idx])
    assert same_bits(res.gradients.cpu().numpy(), rg[np.arange(5), idx])


# ---------------------------------------------------------------- edge cases
def deepest_voxel_centre(c):
    v = c._view
    k = int(torch.argmin(c._packed[:, 0]))
    ijk = np.unravel_index(k, tuple(v.shape))
    return np.array([float(v.dmin[d]) + ijk[d] * float(v.dres[d]) for d in range(3)]), k


def two_placements(leaf):
    m = torch.eye(4).repeat(2 * 2, 1, 1)
    m[2:, 0, 3] = 0.05  # leaf 1 shifted
    comp = pv.ComposedSDF([leaf, leaf], None)
    comp.set_transforms(m.cuda(), batch_dim=(2,))
    return comp


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_exact_ties_in_one_voxel(cache, cache_tri, tri):
    leaf = cache_tri if tri else cache
    centre, _ = deepest_voxel_centre(leaf)
    res = float(leaf._view.dres[0])
    g = torch.Generator().manual_seed(3)
    cluster = torch.tensor(centre, dtype=torch.float32) + (torch.rand(2000, 3, generator=g) - 0.5) * (0.2 * res)
    if tri:  # interpolated values differ inside a voxel: exact duplicates make the ties
        cluster = cluster[:1].repeat(2000, 1)
    pts = torch.cat((c3_pts(5000, seed=2).cpu(), cluster, cluster)).cuda()
    comp = two_placements(leaf)
    for per_leaf in (False, True):
        r = check(comp, pts, per_leaf)
    v, _ = comp(pts)
    assert int((v[0] == v[0].min()).sum()) > 1  # a real tie was decided


def test_nan_record_and_signed_zero():
    leaf = W.build_c2_cache()
    centre, k = deepest_voxel_centre(leaf)
    pts = torch.cat((c3_pts(3000, seed=4), torch.tensor(centre, dtype=torch.float32, device="cuda").view(1, 3).repeat(3, 1)))
    comp = two_placements(leaf)
    with torch.no_grad():
        leaf._packed[k, 0] = float("nan")
    for per_leaf in (False, True):
        r = check(comp, pts, per_leaf)
    assert torch.isnan(r.values[:, 0]).all() and int(r.indices[0, 0]) == 3000
    # -0.0 / +0.0: every record 1.0 except two voxels holding -0.0 and +0.0 -- they tie, the smaller index wins
    with torch.no_grad():
        leaf._packed[:, 0] = 1.0
        leaf._packed[k, 0] = -0.0
        k2 = k + 1
        leaf._packed[k2, 0] = 0.0
    v = leaf._view
    ijk2 = np.unravel_index(k2, tuple(v.shape))
    c2 = [float(v.dmin[d]) + ijk2[d] * float(v.dres[d]) for d in range(3)]
    zpts = torch.tensor([c2, centre.tolist(), c2, centre.tolist()], dtype=torch.float32, device="cuda")
    for order in (zpts, zpts.flip(0)):
        for per_leaf in (False, True):
            r = check(comp, order, per_leaf)
        assert int(r.indices[0, 0]) == 0 and float(r.values[0, 0]) == 0.0


def test_all_out_of_range_one_point_and_ragged_sizes(cache, cache_tri):
    for leaf in (cache, cache_tri):
        comp = c3(leaf, A=2, seed=5)
        far = W.uniform_points_device(1000, [2.0] * 3, [3.0] * 3, seed=6)
        for per_leaf in (False, True):
            check(comp, far, per_leaf)
            check(comp, c3_pts(1, seed=7), per_leaf)
            check(comp, c3_pts(1, seed=7)[0], per_leaf)  # a single (3,) point
            check(comp, c3_pts(4096 + 37, seed=8).reshape(-1, 1, 3), per_leaf)
            check(comp, c3_pts(1000 + 37, seed=9), per_leaf)


def test_many_chunks(cache):
    comp = c3(cache, A=2, seed=10)
    pts = c3_pts(3_000_000, seed=11)  # 733 partial keys per pair
    check(comp, pts, False)
    check(comp, pts[:400_000], True)


def test_generic_fallback_same_contract(cache, cache_tri):
    pts = c3_pts(20_000, seed=12)
    m = W.random_rigid(3 * 2, seed=13, trans=0.2).cuda()
    for leaves in ([cache, pv.SphereSDF(0.05), cache], [cache, cache_tri, cache]):  # a non-grid leaf; mixed modes
        comp = pv.ComposedSDF(leaves, None)
        comp.set_transforms(m, batch_dim=(2,))
        assert comp._fused_mode() is None
        for per_leaf in (False, True):
            check(comp, pts, per_leaf)
    # float16 points take the generic path too, in the dtype __call__ returns
    comp = c3(cache, A=2)
    r = comp.min_over_points(pts.half())
    assert r.values.dtype == comp(pts.half())[0].dtype


# ---------------------------------------------------------------- reproducibility, autograd
def loss_of(values, gradients, seed):
    g = torch.Generator().manual_seed(seed)
    wv = torch.randn(values.shape, generator=g, dtype=torch.float64).to(values)
    wg = torch.randn(gradients.shape, generator=g, dtype=torch.float64).to(gradients)
    return (values * wv).sum() + (gradients * wg).sum()


def gather(v, g, idx, per_leaf_s=None):
    A = idx.shape[0]
    v, g = v.reshape(A, -1), g.reshape(A, -1, 3)
    return v.gather(1, idx.view(A, 1)).squeeze(1), g.gather(1, idx.view(A, 1, 1).expand(A, 1, 3)).squeeze(1)


def close(got, want, rel=1e-5):
    scale = float(want.abs().max()) + 1e-30
    return float((got - want).abs().max()) <= rel * scale


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_robot_dq_matches_autograd_through_call(robot, robot_tri, tri, dtype):
    """Rounding bound: relative 1e-5 of the largest entry (float32), 1e-12 (float64).  Both sides run the same per-pair statements;
    they differ only in how the zero contributions of unselected pairs are added and in the float64 chain VJP."""
    r = robot_tri if tri else robot
    A = 12
    q0 = W.c4_joint_configs(A, seed=21).cuda()
    pts = W.c4_points(20_000, seed=22).to(dtype)
    rel = 1e-5 if dtype == torch.float32 else 1e-12
    for per_leaf in (False, True):
        q = q0.clone().requires_grad_()
        r.set_joint_configuration(q)
        res = r.min_over_points(pts, per_leaf=per_leaf)
        (dq,) = torch.autograd.grad(loss_of(res.values, res.gradients, 1), q)
        q2 = q0.clone().requires_grad_()
        r.set_joint_configuration(q2)
        if per_leaf:
            vs, gs = [], []
            for s in range(len(r.sdf.sdfs)):
                one = pv.ComposedSDF([r.sdf.sdfs[s]], None)
                one.set_transforms(r.sdf._tf_matrix[r.sdf.ith_transform_slice(s)], batch_dim=(A,), known_rigid=True)
                v, g = gather(*one(pts), res.indices[:, s])
                vs.append(v)
                gs.append(g)
            v, g = torch.stack(vs, 1), torch.stack(gs, 1)
        else:
            v, g = gather(*r(pts), res.indices)
        assert same_bits(v.detach().cpu().numpy(), res.values.detach().cpu().numpy())
        (dq_ref,) = torch.autograd.grad(loss_of(v, g, 1), q2)
        assert float(dq_ref.abs().max()) > 0
        assert close(dq, dq_ref, rel), (dq, dq_ref)
        # two backward calls: the same bits
        q3 = q0.clone().requires_grad_()
        r.set_joint_configuration(q3)
        res3 = r.min_over_points(pts, per_leaf=per_leaf)
        (dq3,) = torch.autograd.grad(loss_of(res3.values, res3.gradients, 1), q3)
        assert torch.equal(dq3, dq)
    r.set_joint_configuration(q0)


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_composed_dpoints_dtf(cache, cache_tri, tri):
    comp = c3(cache_tri if tri else cache, A=4, seed=30)
    tfm = comp._tf_matrix.detach().clone()
    for per_leaf in (False, True):
        for dtype in (torch.float32, torch.float64):
            p = c3_pts(8000, seed=31).to(dtype).requires_grad_()
            t = tfm.to(dtype).clone().requires_grad_()
            comp.set_transforms(t, batch_dim=(4,))
            res = comp.min_over_points(p, per_leaf=per_leaf)
            dp, dt = torch.autograd.grad(loss_of(res.values, res.gradients, 2), (p, t))
            res_b = comp.min_over_points(p, per_leaf=per_leaf)
            dp_b, dt_b = torch.autograd.grad(loss_of(res_b.values, res_b.gradients, 2), (p, t))
            assert torch.equal(dp, dp_b) and torch.equal(dt, dt_b)
            # reference: autograd through __call__ (per leaf: one-leaf compositions) gathered at the indices
            if per_leaf:
                vs, gs = [], []
                for s in range(8):
                    one = pv.ComposedSDF([comp.sdfs[s]], None)
                    one.set_transforms(t[comp.ith_transform_slice(s)], batch_dim=(4,), known_rigid=True)
                    v, g = gather(*one(p), res.indices[:, s])
                    vs.append(v)
                    gs.append(g)
                v, g = torch.stack(vs, 1), torch.stack(gs, 1)
            else:
                v, g = gather(*comp(p), res.indices)
            rp, rt = torch.autograd.grad(loss_of(v, g, 2), (p, t))
            rel = 1e-5 if dtype == torch.float32 else 1e-12
            assert close(dp, rp, rel) and close(dt, rt, rel)
            # rows no pair selected: exactly zero
            sel = torch.zeros(p.shape[0], dtype=torch.bool, device="cuda")
            sel[res.indices.reshape(-1)] = True
            assert torch.equal(dp[~sel], torch.zeros_like(dp[~sel]))
            if tri:  # a nearest leaf in range is a table lookup: no derivative w.r.t. the point there
                assert float(dp[sel].abs().max()) > 0
            assert float(dt.abs().max()) > 0
            assert torch.equal(dt[:, 3], torch.zeros_like(dt[:, 3]))
    comp.set_transforms(tfm, batch_dim=(4,))


def test_reproducible_forward(robot):
    robot.set_joint_configuration(W.c4_joint_configs(50, seed=40).cuda())
    pts = W.c4_points(100_000, seed=41)
    for per_leaf in (False, True):
        a = robot.min_over_points(pts, per_leaf=per_leaf)
        b = robot.min_over_points(pts, per_leaf=per_leaf)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ---------------------------------------------------------------- memory, graph capture
def test_peak_memory_c4(robot):
    """A = 200, P = 262,144: the call raises the peak by at most 4 MiB (the outputs, 16 B x 200 x 64 partial keys); the field would
    be A P 4 = 210 MB for the values alone."""
    A, P = 200, 262_144
    robot.set_joint_configuration(W.c4_joint_configs(A, seed=0).cuda())
    pts = W.c4_points(P, seed=1)
    robot.min_over_points(pts)  # descriptors built
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = robot.min_over_points(pts, per_leaf=True)
    res = robot.min_over_points(pts)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 4 << 20
    assert res.values.shape == (A,)


# ---------------------------------------------------------------- more configurations than gridDim.y holds
MANY = H.GRID_Y_MAX + 66  # mop_partial_kernel wraps a += gridDim.y: rows 65535.. are a block's second turn, over the same LDS
EDGE_ROWS = (0, 1, H.GRID_Y_MAX - 1, H.GRID_Y_MAX, H.GRID_Y_MAX + 1, MANY - 1)


def many_configurations(leaf, seed=21):
    """(the composition of two leaves under MANY configurations, the same leaves under the EDGE_ROWS configurations only)"""
    tfm = W.random_rigid(2 * MANY, seed=seed, trans=0.2).reshape(2, MANY, 4, 4)
    comp = pv.ComposedSDF([leaf] * 2, None)
    comp.set_transforms(tfm.reshape(-1, 4, 4).cuda(), batch_dim=(MANY,))
    few = pv.ComposedSDF([leaf] * 2, None)
    few.set_transforms(tfm[:, list(EDGE_ROWS)].reshape(-1, 4, 4).cuda(), batch_dim=(len(EDGE_ROWS),))
    return comp, few


@pytest.mark.parametrize("mode", ["f32-nearest", "f32-trilinear", "f64-nearest"])
@pytest.mark.parametrize("per_leaf", [False, True], ids=["overall", "per_leaf"])
def test_more_configurations_than_grid_rows(cache, cache_tri, mode, per_leaf):
    comp, few = many_configurations(cache_tri if mode == "f32-trilinear" else cache)
    pts = c3_pts(5, seed=22).to(torch.float64 if mode == "f64-nearest" else torch.float32)
    res = check(comp, pts, per_leaf)  # every configuration against __call__ + the restated rule
    assert res.values.shape == ((MANY, 2) if per_leaf else (MANY,))
    # and the rows on either side of the wrap against a composition of those six configurations alone: no launch of it wraps
    ev, ei, eg = expected(few, pts, per_leaf)
    rows = list(EDGE_ROWS)
    assert np.array_equal(res.indices[rows].cpu().numpy(), ei)
    assert same_bits(res.values[rows].cpu().numpy(), ev) and same_bits(res.gradients[rows].cpu().numpy(), eg)
    assert len(np.unique(res.values.cpu().numpy())) > 1000  # the configurations do differ


def test_graph_capture_single_stream(robot):
    robot.set_joint_configuration(W.c4_joint_configs(20, seed=50).cuda())
    pts = W.c4_points(50_000, seed=51)
    eager = robot.min_over_points(pts)
    eager_l = robot.min_over_points(pts, per_leaf=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = robot.min_over_points(pts)
        cap_l = robot.min_over_points(pts, per_leaf=True)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(tuple(eager) + tuple(eager_l), tuple(cap) + tuple(cap_l)):
        assert torch.equal(x, y)
