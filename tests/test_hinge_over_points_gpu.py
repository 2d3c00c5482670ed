"""-m gpu: ComposedSDF / RobotSDF.hinge_over_points (csrc/hinge_over_points.hip, the HINGE policy of composed_backward_kernel)
against the contract of include/pvamd.h "Hinge penalty over points": values within the stated bound of math.fsum over the terms
the torch expression forms from composed(points) (per leaf: one-leaf compositions), counts exact, chunk edges, edge records,
gradients bit for bit against autograd through ((m - composed(points)[0]).clamp(min=0) ** power).sum(-1), the generic path,
peak memory and graph capture."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from tests import helpers as H
from tests.test_interp_gpu import build_robot
from tests.test_min_over_points_gpu import (EDGE_ROWS, c3, c3_pts, deepest_voxel_centre, many_configurations, one_leaf,
                                            two_placements)

pytestmark = pytest.mark.gpu


def batch_of(comp):
    return tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()


def field(comp, pts, per_leaf):
    """(A, Z, P) values of composed(points) (per leaf: the one-leaf compositions), on the host, in the query dtype."""
    with torch.no_grad():
        if per_leaf:
            return np.stack([field(one_leaf(comp, s), pts, False)[:, 0] for s in range(len(comp.sdfs))], axis=1)
        v = comp(pts)[0]
    return v.reshape(math.prod(batch_of(comp)), 1, -1).cpu().numpy()


def expected(v, margin, power):
    """(values, counts, bound) from the (A, Z, P) field: the terms as torch rounds them, summed exactly (math.fsum)."""
    t = torch.from_numpy(v)
    terms = ((margin - t).clamp(min=0) ** power).numpy().astype(np.float64)
    exact = np.array([[math.fsum(r) for r in row] for row in terms])
    counts = (t < margin).sum(-1).numpy()
    if v.dtype == np.float32:
        want = exact.astype(np.float32)
        bound = np.spacing(np.abs(want))  # 1 ulp of the rounded exact sum
    else:
        want = exact
        bound = v.shape[-1] * 2.0 ** -53 * exact
    return want, counts, bound


def check(comp, pts, margin, power, per_leaf):
    res = comp.hinge_over_points(pts, margin, power=power, per_leaf=per_leaf)
    assert isinstance(res, pv.HingeOverPoints)
    batch = batch_of(comp)
    shape = batch + ((len(comp.sdfs),) if per_leaf else ())
    assert res.values.shape == shape and res.counts.shape == shape and res.counts.dtype == torch.int64
    v = field(comp, pts, per_leaf)
    assert res.values.dtype == torch.from_numpy(v).dtype
    want, counts, bound = expected(v, margin, power)
    got = res.values.reshape(want.shape).cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.all(np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64)) <= bound[~nan]), (got, want)
    assert np.array_equal(res.counts.reshape(counts.shape).cpu().numpy(), counts)
    return res, v


def margins(v):
    """Margins below every value (no pair counted), at the median (some) and above every value (all)."""
    f = v[np.isfinite(v)]
    return [float(f.min()) - 0.01, float(np.median(f)), float(f.max()) + 0.01]


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


# ---------------------------------------------------------------- values and counts
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("per_leaf", [False, True], ids=["overall", "per_leaf"])
def test_c3_and_c4_values_and_counts(cache, cache_tri, robot, robot_tri, tri, dtype, per_leaf):
    comp = c3(cache_tri if tri else cache)
    pts = c3_pts(20_000, seed=1).to(dtype)
    v = field(comp, pts, per_leaf)
    for power in (1, 2):
        for m in margins(v):
            check(comp, pts, m, power, per_leaf)
    r = robot_tri if tri else robot
    r.set_joint_configuration(W.c4_joint_configs(8, seed=3).cuda())
    pts = W.c4_points(20_000, seed=5).to(dtype)
    v = field(r.sdf, pts, per_leaf)
    for power in (1, 2):
        for m in margins(v):
            res, _ = check(r.sdf, pts, m, power, per_leaf)
            rr = r.hinge_over_points(pts, m, power=power, per_leaf=per_leaf)  # the robot method is the composition's
            assert torch.equal(rr.values, res.values) and torch.equal(rr.counts, res.counts)
        assert int(res.counts.min()) == 20_000  # the last margin lies above every value
    # some pairs, not all: the median margin
    res = r.hinge_over_points(pts, margins(v)[1], per_leaf=per_leaf)
    assert 0 < int(res.counts.sum()) < res.counts.numel() * 20_000


def test_two_dimensional_batch(cache):
    comp = pv.ComposedSDF([cache] * 3, None)
    comp.set_transforms(W.random_rigid(3 * 6, seed=7, trans=0.2).cuda(), batch_dim=(2, 3))
    pts = c3_pts(9000, seed=8)
    for per_leaf in (False, True):
        res, _ = check(comp, pts, 0.02, 2, per_leaf)
        assert res.values.shape == ((2, 3, 3) if per_leaf else (2, 3))


# ---------------------------------------------------------------- chunk edges, reproducibility
def test_chunk_edges_and_repeats(cache, cache_tri):
    for leaf in (cache, cache_tri):
        comp = c3(leaf, A=2, seed=5)
        for n in (1, 4095, 4096, 4097, 300_001):
            pts = c3_pts(n, seed=n)
            for per_leaf in (False, True):
                a, _ = check(comp, pts, 0.03, 2, per_leaf)
                b = comp.hinge_over_points(pts, 0.03, per_leaf=per_leaf)
                assert torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
                assert torch.equal(a.counts, b.counts)
        # far out of range: the bounding-box branch, every leaf
        far = W.uniform_points_device(3000, [2.0] * 3, [3.0] * 3, seed=6)
        v = field(comp, far, False)
        for m in margins(v):
            check(comp, far, m, 1, False)
            check(comp, far, m, 2, True)


# ---------------------------------------------------------------- edge records
def test_nan_record_and_value_at_margin():
    leaf = W.build_c2_cache()
    centre, k = deepest_voxel_centre(leaf)
    pts = torch.cat((c3_pts(3000, seed=4), torch.tensor(centre, dtype=torch.float32, device="cuda").view(1, 3)))
    comp = two_placements(leaf)
    # v == float32(margin): not counted and a zero term (nearest leaf in range: the record value exactly)
    with torch.no_grad():
        vc = comp(pts)[0][:, -1]
    m = float(vc[0])
    for power in (1, 2):
        for per_leaf in (False, True):
            check(comp, pts, m, power, per_leaf)
        single = comp.hinge_over_points(pts[-1:], m, power=power)
        assert float(single.values[0]) == 0.0 and int(single.counts[0]) == 0
    # a NaN record: the row is NaN, the point is not counted
    with torch.no_grad():
        leaf._packed[k, 0] = float("nan")
    for per_leaf in (False, True):
        r, _ = check(comp, pts, 0.05, 2, per_leaf)
    assert torch.isnan(r.values[:, 0]).all()
    ok = comp.hinge_over_points(pts[:-1], 0.05, per_leaf=True)
    full = comp.hinge_over_points(pts, 0.05, per_leaf=True)
    assert torch.equal(ok.counts[:, 0], full.counts[:, 0])  # the NaN point adds no count


def test_gradient_at_the_margin_out_of_range(cache):
    """v == m at a point outside the range (the bounding-box branch, a derivative there): clamp passes the gradient, so power 1
    gives -dv/dp and power 2 gives 0."""
    comp = pv.ComposedSDF([cache], None)
    comp.set_transforms(torch.eye(4).view(1, 4, 4).cuda(), batch_dim=(1,))
    hi = [float(r[1]) for r in cache.ranges]
    p0 = torch.tensor([[hi[0] + 0.05, hi[1] + 0.03, hi[2] + 0.04]], device="cuda")  # outside on all three axes
    with torch.no_grad():
        v, g = comp(p0)
    m = float(v.reshape(-1)[0])
    for power, want in ((1, -g.reshape(1, 3)), (2, torch.zeros(1, 3, device="cuda"))):
        p = p0.clone().requires_grad_()
        res = comp.hinge_over_points(p, m, power=power)
        assert float(res.values.detach()[0]) == 0.0 and int(res.counts[0]) == 0
        (dp,) = torch.autograd.grad(res.values.sum(), p)
        assert torch.allclose(dp, want, rtol=1e-6, atol=0), (dp, want)
        pr = p0.clone().requires_grad_()
        ref = ((m - comp(pr)[0]).clamp(min=0) ** power).sum(-1)
        (dr,) = torch.autograd.grad(ref.sum(), pr)
        assert torch.equal(dp, dr)


# ---------------------------------------------------------------- gradients: bit for bit against the unfused autograd path
def weights(shape, seed, like):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 + 0.25).to(like)


def unfused(comp, pts, margin, power):
    return ((margin - comp(pts)[0]).clamp(min=0) ** power).sum(-1)


# wide enough that points outside the grids' ranges (the bounding-box branch, 0.1 of padding) fall inside it: a nearest leaf in
# range has no derivative, so a smaller margin leaves the nearest gradients all zero
GRAD_MARGIN = 0.2


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_robot_dq_bit_identical(robot, robot_tri, tri, dtype):
    r = robot_tri if tri else robot
    A = 12
    q0 = W.c4_joint_configs(A, seed=21).cuda()
    pts = W.c4_points(20_000, seed=22).to(dtype)
    S = len(r.sdf_to_link_name)
    for power in (1, 2):
        q = q0.clone().requires_grad_()
        r.set_joint_configuration(q)
        res = r.hinge_over_points(pts, GRAD_MARGIN, power=power)
        w = weights(res.values.shape, 1, res.values)
        (dq,) = torch.autograd.grad((res.values * w).sum(), q)
        q2 = q0.clone().requires_grad_()
        r.set_joint_configuration(q2)
        (dq_ref,) = torch.autograd.grad((unfused(r, pts, GRAD_MARGIN, power) * w).sum(), q2)
        assert float(dq_ref.abs().max()) > 0
        assert torch.equal(dq, dq_ref), (dq - dq_ref).abs().max()
        # per leaf: a differentiable (A, S) result whose rows are the links'
        q3 = q0.clone().requires_grad_()
        r.set_joint_configuration(q3)
        resl = r.hinge_over_points(pts, GRAD_MARGIN, power=power, per_leaf=True)
        assert resl.values.shape == (A, S)
        (dql,) = torch.autograd.grad((resl.values * weights((A, S), 2, resl.values)).sum(), q3)
        assert torch.isfinite(dql).all() and float(dql.abs().max()) > 0
    r.set_joint_configuration(q0)


@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_composed_dpoints_dtf(cache, cache_tri, tri, dtype):
    comp = c3(cache_tri if tri else cache, A=4, seed=30)
    tfm = comp._tf_matrix.detach().clone()
    S, A = 8, 4
    for power in (1, 2):
        p = c3_pts(12_000, seed=31).to(dtype).requires_grad_()
        t = tfm.to(dtype).clone().requires_grad_()
        comp.set_transforms(t, batch_dim=(A,))
        # per_leaf=False: bit for bit against autograd through the torch expression
        res = comp.hinge_over_points(p, GRAD_MARGIN, power=power)
        w = weights((A,), 3, res.values)
        dp, dt = torch.autograd.grad((res.values * w).sum(), (p, t))
        rp, rt = torch.autograd.grad((unfused(comp, p, GRAD_MARGIN, power) * w).sum(), (p, t))
        assert torch.equal(dt, rt), (dt - rt).abs().max()
        assert torch.equal(dp, rp), (dp - rp).abs().max()
        assert float(dt.abs().max()) > 0 and torch.equal(dt[:, 3], torch.zeros_like(dt[:, 3]))
        # twice: the same bits
        res_b = comp.hinge_over_points(p, GRAD_MARGIN, power=power)
        dp_b, dt_b = torch.autograd.grad((res_b.values * w).sum(), (p, t))
        assert torch.equal(dp, dp_b) and torch.equal(dt, dt_b)
        # per_leaf=True: dtf rows bit for bit those of the one-leaf compositions, dpoints close to their sum
        resl = comp.hinge_over_points(p, GRAD_MARGIN, power=power, per_leaf=True)
        wl = weights((A, S), 4, resl.values)
        dpl, dtl = torch.autograd.grad((resl.values * wl).sum(), (p, t))
        rp_sum = torch.zeros_like(p)
        for s in range(S):
            one = pv.ComposedSDF([comp.sdfs[s]], None)
            one.set_transforms(t[comp.ith_transform_slice(s)], batch_dim=(A,), known_rigid=True)
            rps, rts = torch.autograd.grad((unfused(one, p, GRAD_MARGIN, power) * wl[:, s]).sum(), (p, t))
            rows = comp.ith_transform_slice(s)
            assert torch.equal(dtl[rows], rts[rows]), s
            rp_sum = rp_sum + rps
        scale = float(rp_sum.abs().max()) + 1e-30
        rel = 1e-5 if dtype == torch.float32 else 1e-12
        assert float((dpl - rp_sum).abs().max()) <= rel * scale
        if tri:
            assert float(dpl.abs().max()) > 0
    comp.set_transforms(tfm, batch_dim=(A,))


def test_per_leaf_dpoints_of_more_points_than_the_reduction_grids_have_lanes(cache_tri):
    """The per-leaf backward adds the split rows up (reduce_splits_kernel) and then the leaves' terms (accumulate_kernel), both
    streaming over P x 3 elements: past STREAM_GRID_ITEMS / 3 points a lane takes a second one.  A point's gradient depends on
    no other point: the two halves, neither of which strides, give it within the bound test_composed_dpoints_dtf uses for
    dpoints (the halves may split the configurations otherwise)."""
    S, A, P = 2, 2, H.STREAM_GRID_ITEMS // 3 + 4099
    assert P * 3 > H.STREAM_GRID_ITEMS and (P - P // 2) * 3 < H.STREAM_GRID_ITEMS
    comp = pv.ComposedSDF([cache_tri] * S, None)
    t = W.random_rigid(S * A, seed=33, trans=0.2).cuda().requires_grad_()
    comp.set_transforms(t, batch_dim=(A,))
    pts = c3_pts(P, seed=34)
    wl = None

    def grads(rows):
        nonlocal wl
        p = pts[rows].clone().requires_grad_()
        res = comp.hinge_over_points(p, GRAD_MARGIN, per_leaf=True)
        if wl is None:
            wl = weights((A, S), 4, res.values)
        return torch.autograd.grad((res.values * wl).sum(), (p, t))

    dp, dt = grads(slice(0, P))
    half = P // 2
    (dpa, dta), (dpb, dtb) = grads(slice(0, half)), grads(slice(half, P))
    halves = torch.cat((dpa, dpb))
    scale = float(halves.abs().max())
    assert scale > 0 and float((dp - halves).abs().max()) <= 1e-5 * scale
    assert bool((dp[H.STREAM_GRID_ITEMS // 3:].abs().sum(dim=-1) > 0).any())


# ---------------------------------------------------------------- the generic path
def test_generic_fallback_same_contract(cache, cache_tri):
    pts = c3_pts(20_000, seed=12)
    m = W.random_rigid(3 * 2, seed=13, trans=0.2).cuda()
    scaled = m.clone()
    scaled[:, :3, :3] *= 1.1  # not rigid
    for leaves, tfm in (([cache, pv.SphereSDF(0.05), cache], m), ([cache, cache_tri, cache], m), ([cache] * 3, scaled)):
        comp = pv.ComposedSDF(leaves, None)
        comp.set_transforms(tfm, batch_dim=(2,))
        assert comp._fused_mode() is None
        for per_leaf in (False, True):
            for power in (1, 2):
                check(comp, pts, 0.02, power, per_leaf)
    # differentiable wherever __call__ is: float16 points on a fused composition take the generic path and autograd through
    # the torch expression, summed in float64, gives the gradient of the plain expression
    comp = c3(cache, A=2, seed=14)
    tfm = comp._tf_matrix.detach().clone()
    t = tfm.clone().requires_grad_()
    comp.set_transforms(t, batch_dim=(2,))
    ph = pts.half()
    res = comp.hinge_over_points(ph, GRAD_MARGIN)
    assert res.values.dtype == comp(ph)[0].dtype
    (dt,) = torch.autograd.grad(res.values.sum(), t)
    (rt,) = torch.autograd.grad(unfused(comp, ph, GRAD_MARGIN, 2).sum(), t)
    assert torch.equal(dt, rt) and float(dt.abs().max()) > 0
    comp.set_transforms(tfm, batch_dim=(2,))


# ---------------------------------------------------------------- more configurations than gridDim.y holds
@pytest.mark.parametrize("mode", ["f32-nearest", "f32-trilinear", "f64-nearest"])
@pytest.mark.parametrize("per_leaf", [False, True], ids=["overall", "per_leaf"])
def test_more_configurations_than_grid_rows(cache, cache_tri, mode, per_leaf):
    """hop_partial_kernel wraps a += gridDim.y and reuses its LDS partials behind a trailing barrier: rows 65535.. are a block's
    second turn."""
    comp, few = many_configurations(cache_tri if mode == "f32-trilinear" else cache)
    pts = c3_pts(5, seed=22).to(torch.float64 if mode == "f64-nearest" else torch.float32)
    v = field(comp, pts, per_leaf)
    m = margins(v)[1]
    rows = list(EDGE_ROWS)
    for power in (1, 2):
        res, _ = check(comp, pts, m, power, per_leaf)  # every configuration against composed(points), summed exactly
        counts = res.counts.cpu().numpy()
        assert ((counts > 0) & (counts < 5)).any() and (counts == 0).any()  # the margin cuts through the rows
        # the rows on either side of the wrap against a composition of those six configurations alone: no launch of it wraps
        want, wcounts, bound = expected(field(few, pts, per_leaf), m, power)
        got = res.values[rows].reshape(want.shape).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want.astype(np.float64)) <= bound), (got, want)
        assert np.array_equal(counts[rows].reshape(wcounts.shape), wcounts)


# ---------------------------------------------------------------- memory, graph capture
def test_peak_memory_c4(robot):
    """A = 200, P = 262,144, forward and backward to q: at most 64 MiB above the baseline (the backward's plan scratch is about
    20 MB); the unfused step allocates the (A, P) field, its gradient field and the torch temporaries, over 1.2 GB."""
    A, P = 200, 262_144
    q0 = W.c4_joint_configs(A, seed=0).cuda()
    pts = W.c4_points(P, seed=1)

    def step():
        q = q0.clone().requires_grad_()
        robot.set_joint_configuration(q)
        res = robot.hinge_over_points(pts, 0.02)
        res.values.sum().backward()
        return q.grad

    step()  # descriptors built
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = step()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20
    assert torch.isfinite(g).all()


def test_graph_capture_single_stream(robot):
    robot.set_joint_configuration(W.c4_joint_configs(20, seed=50).cuda())
    pts = W.c4_points(50_000, seed=51)
    eager = robot.hinge_over_points(pts, 0.02)
    eager_l = robot.hinge_over_points(pts, 0.02, power=1, per_leaf=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = robot.hinge_over_points(pts, 0.02)
        cap_l = robot.hinge_over_points(pts, 0.02, power=1, per_leaf=True)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(tuple(eager) + tuple(eager_l), tuple(cap) + tuple(cap_l)):
        assert torch.equal(x, y)
