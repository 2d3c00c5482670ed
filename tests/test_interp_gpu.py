"""-m gpu: interpolation="trilinear" (csrc/lane_query.hip, the interpolated leaf of csrc/backward.hip) against the CPU restatement of
its arithmetic contract (tests/interp_ref.c: bit for bit) and, for gradients, float64 torch autograd through the same
expressions given the kernel's decisions.  The gradient checks here keep away from cell, range and box faces; the backward's
behaviour AT those edges is held to a worst-case bound in tests/test_interp_edges_gpu.py."""
import ctypes
import math
import tempfile

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from tests import helpers as H
from tests import interp_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4  # relative to res: points this close to a cell face, range face or box face are kept out of gradient checks


@pytest.fixture(scope="module")
def nearest():
    return W.build_c2_cache()


@pytest.fixture(scope="module")
def tri():
    c = W.build_c2_cache()
    c.interpolation = "trilinear"
    return c


def build_robot(**kw):
    with tempfile.TemporaryDirectory() as tmp:
        chain = W.synthetic_arm(tmp)
        return pv.RobotSDF(chain, path_prefix=tmp, link_sdf_cls=pv.cache_link_sdf_factory(0.02, 0.1, device="cuda", cache_path=None,
                                                                                             **kw))


@pytest.fixture(scope="module")
def robot():
    return build_robot(interpolation="trilinear")


@pytest.fixture(scope="module")
def robot_nearest():
    return build_robot()


def desc_with_rule(c, rule):
    d = _lib.GridDesc.from_buffer_copy(bytes(c._grid_desc()))
    d.rule = rule
    _lib.check(_lib.load().pvamd_grid_finalize(ctypes.byref(d)), "pvamd_grid_finalize")
    return d


def run_abi(name, desc, pts):
    """(val, grad, oob) of one cached entry point on a descriptor."""
    lib = _lib.load()
    P = pts.shape[0]
    val = torch.empty((P,), dtype=pts.dtype, device=pts.device)
    grad = torch.empty((P, 3), dtype=pts.dtype, device=pts.device)
    oob = torch.empty((P,), dtype=torch.uint8, device=pts.device)
    f = getattr(lib, name + ("_f64" if pts.dtype == torch.float64 else ""))
    _lib.check(f(ctypes.byref(desc), _lib.ptr(pts), P, _lib.ptr(val), _lib.ptr(grad), _lib.ptr(oob), _lib.stream_ptr()), name)
    torch.cuda.synchronize()
    return val.cpu().numpy(), grad.cpu().numpy(), oob.cpu().numpy()


def edge_points(c, rule):
    """Points exactly on cell faces, on voxel centres and on the range faces (and half a voxel beyond, which is valid under
    PVAMD_RULE_VALID_ON_INDEX), plus non-finite points."""
    v = c._view
    mn, res, shape = np.array([float(a) for a in v.dmin]), np.array([float(a) for a in v.dres]), np.array(v.shape)
    rng = np.random.default_rng(7)
    k = rng.integers(0, shape - 1, size=(3000, 3))
    centres = mn + k * res
    faces = mn + (k + 0.5) * res
    lo_face, hi_face = mn + 0 * k, mn + (shape - 1) * res + 0 * k
    out = [centres, faces]
    for d in range(3):
        for edge in (lo_face, hi_face):
            for shift in (0.0, -0.5, 0.5, -0.4999, 0.4999):
                p = centres.copy()[:500]
                p[:, d] = edge[:500, d] + shift * res[d]
                out.append(p)
    bad = centres[:6].copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    bad[3] = np.nan
    bad[4, 0] = 1e30
    bad[5, 2] = -1e30
    out.append(bad)
    return np.concatenate(out)


def point_sets(c):
    return np.concatenate([W.c2_points(c, 200_000, seed=11).cpu().double().numpy(),               # headline mix
                           W.c2_points(c, 100_000, seed=12, margin=-0.02).cpu().double().numpy(),  # all in range
                           edge_points(c, 0)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rule", [0, _lib.RULE_VALID_ON_INDEX if hasattr(_lib, "RULE_VALID_ON_INDEX") else 1])
def test_cached_forward_bit_exact(nearest, tri, dtype, rule):
    pts = torch.from_numpy(point_sets(tri)).to(dtype).cuda().contiguous()
    f64 = dtype == torch.float64
    for mode in (pv.OutOfBoundsStrategy.BOUNDING_BOX, pv.OutOfBoundsStrategy.LOOKUP_GT_SDF):
        d = _lib.GridDesc.from_buffer_copy(bytes(tri._grid_desc(mode)))
        d.rule = rule
        _lib.check(_lib.load().pvamd_grid_finalize(ctypes.byref(d)), "finalize")
        nv, ng, noob = run_abi("pvamd_cached_query", d, pts)
        tv, tg, toob = run_abi("pvamd_cached_query_interp", d, pts)
        assert np.array_equal(noob, toob), "range decision differs from the nearest mode's"
        out = toob == 1
        assert out.sum() > 1000 and (~out).sum() > 1000
        # out of range: the nearest mode's outputs, bit for bit
        assert np.array_equal(nv[out], tv[out], equal_nan=True) and np.array_equal(ng[out], tg[out], equal_nan=True)
        rec, shape, mn, res = R.grid_numbers(tri, f64)
        rv, rg = R.forward(rec, shape, mn, res, pts.cpu().numpy(), ~out)
        assert np.array_equal(rv[~out], tv[~out]) and np.array_equal(rg[~out], tg[~out])
        if mode == pv.OutOfBoundsStrategy.BOUNDING_BOX:
            box = tv, tg
    # the public call is the same entry point
    if rule == 0:
        tv, tg = box
        val, grad = tri(pts)
        assert np.array_equal(val.cpu().numpy(), tv, equal_nan=True) and np.array_equal(grad.cpu().numpy(), tg, equal_nan=True)
        nval, _ = nearest(pts)
        assert not np.array_equal(nval.cpu().numpy()[~out], tv[~out])


def test_continuity_along_lines(nearest, tri):
    v = tri._view
    lo = np.array([float(a) for a in v.dmin]) + 1e-3
    hi = np.array([float(a) for a in v.dmax]) - 1e-3
    rng = np.random.default_rng(3)
    n = 20001
    t = np.linspace(0, 1, n)
    rec = tri._packed.cpu().numpy()
    res = float(v.dres.min())
    shape = np.array(v.shape)
    # slope bound of the interpolant along a unit direction: the largest record difference between neighbours per voxel
    val = rec[:, 0].reshape(*shape)
    slope = max(np.abs(np.diff(val, axis=d)).max() for d in range(3)) / res * math.sqrt(3)
    for _ in range(4):
        a, b = lo + rng.random(3) * (hi - lo), lo + rng.random(3) * (hi - lo)
        line = torch.from_numpy(a + t[:, None] * (b - a)).float().cuda()
        step = float(np.linalg.norm(b - a)) / (n - 1)
        tv = tri(line)[0].cpu().numpy().astype(np.float64)
        nv = nearest(line)[0].cpu().numpy().astype(np.float64)
        assert np.abs(np.diff(tv)).max() <= slope * step * 1.01 + 1e-5
        assert np.abs(np.diff(nv)).max() > slope * step * 10  # the nearest mode jumps at half-voxel planes


def stable_leaf(c, x):
    """x (..., 3) float64 leaf frame: TOL * res away from cell faces, range faces and surface-box faces."""
    v = c._view
    mn = torch.tensor([float(a) for a in v.dmin], dtype=torch.float64, device=x.device)
    mx = torch.tensor([float(a) for a in v.dmax], dtype=torch.float64, device=x.device)
    res = torch.tensor([float(a) for a in v.dres], dtype=torch.float64, device=x.device)
    bb = c.bb.double().to(x.device)
    q = (x - mn) / res
    ok = ((q - q.round()).abs() > TOL).all(-1)
    ok &= ((x - mn).abs() > TOL * res).all(-1) & ((x - mx).abs() > TOL * res).all(-1)
    ok &= ((x - bb[:, 0]).abs() > TOL * res).all(-1) & ((x - bb[:, 1]).abs() > TOL * res).all(-1)
    return ok


def inside_leaf(c, x):
    v = c._view
    mn = torch.tensor([float(a) for a in v.dmin], dtype=torch.float64, device=x.device)
    mx = torch.tensor([float(a) for a in v.dmax], dtype=torch.float64, device=x.device)
    return ((mn <= x) & (x <= mx)).all(-1)


def composed_ref_f32(leaves, tfm, pts):
    """interp_ref.c's composed_forward_f32 over the leaves' own descriptors."""
    lib = R.load()
    S = len(leaves)
    A = tfm.shape[0] // S
    P = pts.shape[0]
    descs = [c._grid_desc() for c in leaves]
    recs = [np.ascontiguousarray(c._packed.cpu().numpy()) for c in leaves]
    arr = lambda rows, dt: np.ascontiguousarray(np.array(rows, dt))
    shapes = arr([list(d.shape) for d in descs], np.int32)
    mns, ress = arr([list(d.fmin) for d in descs], np.float32), arr([list(d.fres) for d in descs], np.float32)
    vlos, vhis = arr([list(d.vlo) for d in descs], np.float32), arr([list(d.vhi) for d in descs], np.float32)
    bbs = arr([list(d.bb_min) + list(d.bb_max) for d in descs], np.float32)
    ptrs = (ctypes.c_void_p * S)(*[r.ctypes.data for r in recs])
    tf_np = np.ascontiguousarray(tfm.detach().cpu().numpy().astype(np.float32))
    p_np = np.ascontiguousarray(pts.cpu().numpy().astype(np.float32))
    val = np.empty((A, P), np.float32)
    grad = np.empty((A, P, 3), np.float32)
    leaf = np.empty((A, P), np.int32)
    lib.composed_forward_f32(ctypes.c_int32(S), ptrs, R._p(shapes), R._p(mns), R._p(ress), R._p(vlos), R._p(vhis), R._p(bbs),
                             R._p(tf_np), ctypes.c_int32(A), R._p(p_np), ctypes.c_int64(P), R._p(val), R._p(grad), R._p(leaf))
    return val, grad, leaf


def composed_ref_f64(leaves, tfm, pts):
    """interp_ref.c's composed_forward_f64 over the leaves' own descriptors."""
    lib = R.load()
    S = len(leaves)
    A = tfm.shape[0] // S
    P = pts.shape[0]
    descs = [c._grid_desc() for c in leaves]
    recs = [np.ascontiguousarray(c._packed.cpu().numpy()) for c in leaves]
    arr = lambda rows, dt: np.ascontiguousarray(np.array(rows, dt))
    shapes = arr([list(d.shape) for d in descs], np.int32)
    mns, ress = arr([list(d.dmin) for d in descs], np.float64), arr([list(d.dres) for d in descs], np.float64)
    dmins, dmaxs = arr([list(d.dmin) for d in descs], np.float64), arr([list(d.dmax) for d in descs], np.float64)
    bbs = arr([list(d.dbb_min) + list(d.dbb_max) for d in descs], np.float64)
    ptrs = (ctypes.c_void_p * S)(*[r.ctypes.data for r in recs])
    tf_np = np.ascontiguousarray(tfm.detach().cpu().numpy().astype(np.float64))
    p_np = np.ascontiguousarray(pts.cpu().numpy().astype(np.float64))
    val = np.empty((A, P), np.float64)
    grad = np.empty((A, P, 3), np.float64)
    leaf = np.empty((A, P), np.int32)
    lib.composed_forward_f64(ctypes.c_int32(S), ptrs, R._p(shapes), R._p(mns), R._p(ress), R._p(dmins), R._p(dmaxs), R._p(bbs),
                             R._p(tf_np), ctypes.c_int32(A), R._p(p_np), ctypes.c_int64(P), R._p(val), R._p(grad), R._p(leaf))
    return val, grad, leaf


def robot_points(n, seed):
    return W.c4_points(n, seed=seed)


def test_composed_and_robot_forward_bit_exact(robot, robot_nearest):
    q = W.c4_joint_configs(6, seed=2).cuda()
    robot.set_joint_configuration(q)
    pts = robot_points(20000, seed=4)
    pts = torch.cat((pts, torch.tensor([[math.nan, 0, 0], [math.inf, 0, 0]], device="cuda")))
    val, grad = robot(pts)
    comp = robot.sdf
    tfm = comp._tf_matrix
    rv, rg, rl = composed_ref_f32(comp.sdfs, tfm, pts)
    assert np.array_equal(val.cpu().numpy(), rv, equal_nan=True)
    assert np.array_equal(grad.cpu().numpy(), rg, equal_nan=True)
    _, _, leaf, _, _ = comp._interp_forward(pts, want_leaf=True)
    assert np.array_equal(leaf.cpu().numpy(), rl)
    # a ComposedSDF over the same leaves and stack answers the same
    same = pv.ComposedSDF(comp.sdfs, None)
    same.set_transforms(tfm.clone(), batch_dim=(6,))
    v2, g2 = same(pts)
    assert torch.equal(v2, val) and torch.equal(torch.nan_to_num(g2, 7.0), torch.nan_to_num(grad, 7.0))
    # and it is not the nearest robot (the routing reached the trilinear kernel)
    robot_nearest.set_joint_configuration(q)
    nv, _ = robot_nearest(pts)
    assert not torch.equal(nv, val)
    # float64: the f64 kernel, range in float64, against the f32 answer within rounding
    v64, _ = robot(pts[:-2].double())
    assert v64.dtype == torch.float64
    assert torch.allclose(v64.float(), val[:, :-2], atol=1e-5, rtol=1e-5)


def test_composed_forward_with_more_configurations_than_grid_rows(tri):
    """composed_interp_kernel takes the configuration from blockIdx.y and wraps a += gridDim.y: rows 65535.. are a block's second
    turn.  Values, gradients and leaf ids of every configuration against interp_ref.c, and the rows on either side of the wrap
    again by name."""
    A = H.GRID_Y_MAX + 66
    comp = pv.ComposedSDF([tri, tri], None)
    comp.set_transforms(W.random_rigid(2 * A, seed=61, trans=0.2).cuda(), batch_dim=(A,))
    pts = torch.cat((W.c3_points(4, seed=62), torch.tensor([[math.nan, 0, 0]], device="cuda")))
    assert comp._fused_mode() == "trilinear"
    rv, rg, rl = composed_ref_f32(comp.sdfs, comp._tf_matrix, pts)
    val, grad = comp(pts)
    assert val.shape == (A, 5) and grad.shape == (A, 5, 3)
    _, _, leaf, _, _ = comp._interp_forward(pts, want_leaf=True)
    val, grad, leaf = val.cpu().numpy(), grad.cpu().numpy(), leaf.cpu().numpy()
    assert np.array_equal(val, rv, equal_nan=True) and np.array_equal(grad, rg, equal_nan=True) and np.array_equal(leaf, rl)
    for a in (0, 1, H.GRID_Y_MAX - 1, H.GRID_Y_MAX, H.GRID_Y_MAX + 1, A - 1):
        assert np.array_equal(val[a], rv[a], equal_nan=True) and np.array_equal(grad[a], rg[a], equal_nan=True), a
        assert np.array_equal(leaf[a], rl[a]), a
    assert len(np.unique(val[:, 0])) > 1000 and (rl == 0).any() and (rl == 1).any()  # the rows differ, both leaves answer


def composed_abi_f64(comp, tfm, pts):
    """pvamd_composed_query_interp_f64 over comp's leaves with the float64 stack tfm: (val, grad, leaf) on the host."""
    S = len(comp.sdfs)
    A = tfm.shape[0] // S
    P = pts.shape[0]
    tf64 = tfm.detach().double().cuda().contiguous()
    val = torch.empty((A, P), dtype=torch.float64, device="cuda")
    grad = torch.empty((A, P, 3), dtype=torch.float64, device="cuda")
    leaf = torch.empty((A, P), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().pvamd_composed_query_interp_f64(_lib.ptr(comp._leaf_grids(pts.device)), S, _lib.ptr(tf64), A, _lib.ptr(pts),
                                                           P, _lib.ptr(val), _lib.ptr(grad), _lib.ptr(leaf), _lib.stream_ptr()),
               "pvamd_composed_query_interp_f64")
    torch.cuda.synchronize()
    return val.cpu().numpy(), grad.cpu().numpy(), leaf.cpu().numpy()


def test_composed_forward_f64_bit_exact(robot, tri):
    """The float64 trilinear composed kernel against interp_ref.c's composed_forward_f64: values, gradients and leaf ids, bit for
    bit, on the robot's link caches and on three placements of one cache, with non-finite rows."""
    bad = torch.tensor([[math.nan, 0, 0], [0, math.inf, 0], [0, 0, -math.inf], [math.nan] * 3, [1e300, 0, 0], [0, -1e300, 0]],
                       dtype=torch.float64, device="cuda")
    q = W.c4_joint_configs(5, seed=7).cuda()
    robot.set_joint_configuration(q)
    rpts = torch.cat((robot_points(20000, seed=6).double(), bad)).contiguous()
    A = 3
    placed = pv.ComposedSDF([tri, tri, tri], None)
    placed.set_transforms(W.random_rigid(3 * A, seed=9, trans=0.05).double().cuda(), batch_dim=(A,))
    cpts = torch.cat((W.c2_points(tri, 20000, seed=8).double(), bad)).contiguous()
    for comp, pts in ((robot.sdf, rpts), (placed, cpts)):
        tfm = comp._tf_matrix.detach().double()
        gv, gg, gl = composed_abi_f64(comp, tfm, pts)
        rv, rg, rl = composed_ref_f64(comp.sdfs, tfm, pts)
        assert np.array_equal(gv, rv, equal_nan=True)
        assert np.array_equal(gg, rg, equal_nan=True)
        assert np.array_equal(gl, rl)
        assert len(np.unique(gl)) > 1 and np.isfinite(gv).mean() > 0.9
        # the public float64 call is the same kernel
        val, grad = comp(pts)
        assert np.array_equal(val.reshape(gv.shape).cpu().numpy(), gv, equal_nan=True)
        assert np.array_equal(grad.reshape(gg.shape).cpu().numpy(), gg, equal_nan=True)


# ---------------------------------------------------------------- gradients
def test_gradcheck_cached(tri):
    pts = W.c2_points(tri, 4000, seed=21, margin=-0.02).double()
    pts = pts[stable_leaf(tri, pts)][:200].contiguous()
    x = pts.clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda p: tri(p), (x,), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_gradcheck_composed_points_and_transforms(tri):
    A = 3
    m = W.random_rigid(2 * A, seed=5, trans=0.03).double().cuda()
    comp = pv.ComposedSDF([tri, tri], None)
    pts = W.c2_points(tri, 4000, seed=22, margin=-0.05).double()
    x = (pts.unsqueeze(0) @ m[:, :3, :3].transpose(-1, -2) + m[:, None, :3, 3])
    ok = stable_leaf(tri, x).all(0) & inside_leaf(tri, x).all(0)
    pts = pts[ok][:60].contiguous().requires_grad_()
    mm = m.clone().requires_grad_()

    def f(p, mat):
        comp.set_transforms(mat, batch_dim=(A,))
        return comp(p)

    assert torch.autograd.gradcheck(f, (pts, mm), eps=1e-6, atol=1e-5, rtol=1e-4)


def robot_f64(robot, pts, A):
    """val(q) through the robot's own float64 torch forward kinematics (RobotSDF._stack_torch, what ChainConfigure differentiates)
    and the trilinear composed query: a function gradcheck can perturb (the product path configures in float32)."""
    def f(q):
        robot.sdf.set_transforms(robot._stack_torch(q.reshape(A, -1)), batch_dim=(A,))
        return robot.sdf(pts)[0]
    return f


def winners_in_range(comp, pts, leaf):
    """(A, P) bool: the winning leaf's point lies in its cache's range."""
    S = len(comp.sdfs)
    A = leaf.shape[0]
    m = comp._tf_matrix.detach().double().reshape(S, A, 4, 4)
    ins = torch.stack([inside_leaf(c, pts.double().unsqueeze(0) @ m[s, :, :3, :3].transpose(-1, -2) + m[s, :, None, :3, 3])
                       for s, c in enumerate(comp.sdfs)])
    return ins.gather(0, leaf.long().unsqueeze(0)).squeeze(0)


def stable_points(comp, pts):
    S = len(comp.sdfs)
    A = comp._tf_matrix.shape[0] // S
    m = comp._tf_matrix.detach().double().reshape(S, A, 4, 4)
    ok = torch.ones(pts.shape[0], dtype=torch.bool, device=pts.device)
    for s, c in enumerate(comp.sdfs):
        ok &= stable_leaf(c, pts.double().unsqueeze(0) @ m[s, :, :3, :3].transpose(-1, -2) + m[s, :, None, :3, 3]).all(0)
    return ok


def test_gradcheck_robot_q(robot):
    A = 2
    q0 = W.c4_joint_configs(A, seed=8).cuda().double()
    pts = robot_points(4000, seed=9).double()
    robot.set_joint_configuration(q0)
    with torch.no_grad():
        _, _, leaf, _, _ = robot.sdf._interp_forward(pts, want_leaf=True)
        keep = stable_points(robot.sdf, pts) & winners_in_range(robot.sdf, pts, leaf).all(0)
    pts = pts[keep][:40].contiguous()
    assert pts.shape[0] >= 20
    f = robot_f64(robot, pts, A)
    assert torch.autograd.gradcheck(f, (q0.clone().requires_grad_(),), eps=1e-6, atol=1e-5, rtol=1e-3)
    # the product path (float32 configure + ChainConfigure) gives that gradient to float32 precision
    w = torch.randn(A, pts.shape[0], generator=torch.Generator().manual_seed(3), dtype=torch.float64).cuda()
    q64 = q0.clone().requires_grad_()
    (f(q64) * w).sum().backward()
    q = q0.clone().requires_grad_()
    robot.set_joint_configuration(q)
    (robot(pts)[0] * w).sum().backward()
    assert float(q64.grad.abs().sum()) > 0
    assert torch.allclose(q.grad, q64.grad, rtol=1e-3, atol=1e-3 * float(q64.grad.abs().max()))


def test_float32_vjps_match_float64_restatement(tri):
    # cached
    pts = W.c2_points(tri, 40000, seed=31).double()
    pts = pts[stable_leaf(tri, pts)].contiguous()
    g = torch.Generator().manual_seed(1)
    wv = torch.randn(pts.shape[0], generator=g, dtype=torch.float64).cuda()
    wg = torch.randn(pts.shape[0], 3, generator=g, dtype=torch.float64).cuda()
    p32 = pts.float().requires_grad_()
    v, gr = tri(p32)
    ((v.double() * wv).sum() + (gr.double() * wg).sum()).backward()
    p64 = p32.detach().double().requires_grad_()
    rv, rg = R.leaf_torch(tri, p64, inside_leaf(tri, p64))
    ((rv * wv).sum() + (rg * wg).sum()).backward()
    got, want = p32.grad.double(), p64.grad
    assert (got - want).abs().sum() <= 1e-5 * (want.abs().sum() + got.abs().sum())
    assert int(inside_leaf(tri, pts).sum()) > 1000 and float(got[inside_leaf(tri, pts)].abs().sum()) > 0
    # the C restatement of the per-point VJP
    ins = inside_leaf(tri, pts).cpu().numpy()
    rec, shape, mn, res = R.grid_numbers(tri, False)
    cv = R.vjp(rec, shape, mn.astype(np.float64), res.astype(np.float64), p32.detach().double().cpu().numpy(), ins,
               wv.cpu().numpy(), wg.cpu().numpy())
    gi = got.cpu().numpy()[ins]
    assert np.abs(cv[ins] - gi).sum() <= 1e-5 * (np.abs(cv[ins]).sum() + np.abs(gi).sum())
    # composed: points and transforms
    A, S = 4, 2
    m = W.random_rigid(S * A, seed=6, trans=0.05).cuda()
    comp = pv.ComposedSDF([tri, tri], None)
    mm = m.clone().requires_grad_()
    comp.set_transforms(mm, batch_dim=(A,))
    cp = W.c2_points(tri, 20000, seed=32).cuda()
    x = cp.double().unsqueeze(0) @ m.double()[:, :3, :3].transpose(-1, -2) + m.double()[:, None, :3, 3]
    keep = stable_leaf(tri, x).all(0)
    cp = cp[keep].contiguous().requires_grad_()
    val, grad = comp(cp)
    wv = torch.randn(val.shape, generator=g, dtype=torch.float64).cuda()
    wg = torch.randn(grad.shape, generator=g, dtype=torch.float64).cuda()
    ((val.double() * wv).sum() + (grad.double() * wg).sum()).backward()
    _, _, leaf, _, _ = comp._interp_forward(cp.detach(), want_leaf=True)
    p64 = cp.detach().double().requires_grad_()
    m64 = m.detach().double().requires_grad_()
    x = p64.unsqueeze(0) @ m64[:, :3, :3].transpose(-1, -2) + m64[:, None, :3, 3]
    insides = inside_leaf(tri, x.detach()).reshape(S, A, -1)
    rv, rg = R.composed_torch([tri, tri], m64, p64, leaf, insides)
    ((rv * wv).sum() + (rg * wg).sum()).backward()
    for got, want in ((cp.grad.double(), p64.grad), (mm.grad.double(), m64.grad)):
        assert (got - want).abs().sum() <= 1e-5 * (want.abs().sum() + got.abs().sum())


def test_backward_is_reproducible(tri, robot):
    pts = W.c2_points(tri, 100_000, seed=41).requires_grad_()
    outs = []
    for _ in range(2):
        pts.grad = None
        v, g = tri(pts)
        (v.sum() + g.sum()).backward()
        outs.append(pts.grad.clone())
    assert torch.equal(outs[0], outs[1])
    q = W.c4_joint_configs(16, seed=3).cuda()
    rp = robot_points(50_000, seed=5)
    grads = []
    for _ in range(2):
        qq = q.clone().requires_grad_()
        robot.set_joint_configuration(qq)
        v, g = robot(rp)
        (v.sum() + g.sum()).backward()
        grads.append(qq.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().sum()) > 0


def nearest_leaf_ids(comp, pts):
    S, A = len(comp.sdfs), comp._tf_matrix.shape[0] // len(comp.sdfs)
    P = pts.shape[0]
    val = torch.empty((A, P), device="cuda")
    grad = torch.empty((A, P, 3), device="cuda")
    leaf = torch.empty((A, P), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().pvamd_composed_query(_lib.ptr(comp._leaf_grids(pts.device)), S, _lib.ptr(comp._tf_device(pts.device)), A,
                                                _lib.ptr(pts), P, _lib.ptr(val), _lib.ptr(grad), _lib.ptr(leaf), 0, _lib.stream_ptr()),
               "pvamd_composed_query")
    return leaf


def test_readme_user_story_gives_a_joint_gradient(robot, robot_nearest):
    """The README autograd example with points in range of the link caches: non-zero q.grad that matches gradcheck; the nearest
    leaves give exactly zero there."""
    margin = 0.05
    q0 = W.c4_joint_configs(1, seed=12).cuda()
    pts = robot_points(40000, seed=13)
    robot.set_joint_configuration(q0)
    robot_nearest.set_joint_configuration(q0)
    with torch.no_grad():
        v, _, leaf, _, _ = robot.sdf._interp_forward(pts, want_leaf=True)
        nleaf = nearest_leaf_ids(robot_nearest.sdf, pts)
        keep = stable_points(robot.sdf, pts) & winners_in_range(robot.sdf, pts, leaf)[0] & \
            winners_in_range(robot_nearest.sdf, pts, nleaf)[0] & (v.reshape(-1) < margin)
    pts = pts[keep][:300].contiguous()
    assert pts.shape[0] >= 50

    def cost(r, q):
        r.set_joint_configuration(q)  # q.requires_grad_()
        val, grad = r(pts)
        return ((margin - val).clamp(min=0) ** 2).sum()

    q = q0.clone().requires_grad_()
    cost(robot, q).backward()
    assert float(q.grad.abs().sum()) > 0
    # gradcheck of the same cost through the float64 forward kinematics, and agreement with the product path
    f = robot_f64(robot, pts.double(), 1)
    c64 = lambda qq: ((margin - f(qq)).clamp(min=0) ** 2).sum()
    assert torch.autograd.gradcheck(c64, (q0.double().clone().requires_grad_(),), eps=1e-6, atol=1e-5, rtol=1e-3)
    q64 = q0.double().clone().requires_grad_()
    c64(q64).backward()
    assert torch.allclose(q.grad.double(), q64.grad, rtol=1e-3, atol=1e-3 * float(q64.grad.abs().max()))
    # nearest leaves: in range the lookup has no derivative
    qn = q0.clone().requires_grad_()
    cost(robot_nearest, qn).backward()
    assert qn.grad is not None and float(qn.grad.abs().sum()) == 0.0


# ---------------------------------------------------------------- routing
def test_entry_points_without_trilinear_kernels_raise(tri, robot):
    pts = W.c2_points(tri, 1024, seed=51).contiguous()
    val = torch.empty(1024, device="cuda")
    grad = torch.empty(1024, 3, device="cuda")
    with pytest.raises(ValueError, match="interpolation"):
        tri.query_into(pts, val, grad)
    comp = pv.ComposedSDF([tri, tri], W.random_rigid(2, seed=1).cuda())
    for call in (lambda: comp.query_into(pts, val, grad), lambda: comp.prepare_points(pts), lambda: comp.query_packed(pts),
                 lambda: comp.query_configs(pts, 0, 1)):
        with pytest.raises(ValueError, match="interpolation"):
            call()
    A = 2
    q = W.c4_joint_configs(A, seed=1).cuda()
    with pytest.raises(ValueError, match="interpolation"):
        robot.configure_and_query_into(q, pts, torch.empty(A, 1024, device="cuda"), torch.empty(A, 1024, 3, device="cuda"))
    robot.set_joint_configuration(q)
    with pytest.raises(ValueError, match="interpolation"):
        robot.query_into(pts, torch.empty(A, 1024, device="cuda"), torch.empty(A, 1024, 3, device="cuda"))
    with pytest.raises(ValueError, match="interpolation"):
        robot.prepare_points(pts)


def test_outside_surface_and_mixed_composition(nearest, tri):
    pts = W.c2_points(tri, 50_000, seed=52)
    v, _ = tri(pts)
    _, _, oob = run_abi("pvamd_cached_query_interp", tri._grid_desc(), pts.contiguous())
    want = torch.from_numpy(oob != 0).cuda() | (v > 0.01)
    assert torch.equal(tri.outside_surface(pts, 0.01), want)
    # nearest + trilinear leaves: the generic path, each leaf answering in its own mode
    m = W.random_rigid(2, seed=3, trans=0.02).cuda()
    mixed = pv.ComposedSDF([nearest, tri], m)
    mv, _ = mixed(pts)
    x = [pts @ m[s, :3, :3].T + m[s, :3, 3] for s in range(2)]
    v0, v1 = nearest(x[0])[0], tri(x[1])[0]
    assert torch.allclose(mv, torch.minimum(v0, v1), atol=0, rtol=0)


def test_chamfer_against_a_trilinear_grid(tri):
    B = 4
    params = torch.randn(B, 6, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 0.02
    params[:, 3:] += 0.1
    W32 = torch.eye(4).repeat(B, 1, 1)
    W32[:, :3, 3] = params[:, :3].float()
    Wt = W32.cuda().requires_grad_()
    pts = W.c2_points(tri, 3000, seed=53, margin=-0.03).requires_grad_()
    err = pv.batch_chamfer_dist(Wt, pts, obj_sdf=tri, scale=10.0)
    err.sum().backward()
    # float64 torch restatement
    W64 = Wt.detach().double().requires_grad_()
    p64 = pts.detach().double().requires_grad_()
    x = p64.unsqueeze(0) @ W64[:, :3, :3].transpose(-1, -2) + W64[:, None, :3, 3]
    d, _ = R.leaf_torch(tri, x, inside_leaf(tri, x.detach()))
    ref = ((10.0 * d) ** 2).mean(dim=-1)
    ref.sum().backward()
    assert torch.allclose(err.double(), ref, rtol=1e-5)
    assert torch.allclose(Wt.grad.double(), W64.grad, rtol=1e-4, atol=1e-4 * float(W64.grad.abs().max()))
    assert torch.allclose(pts.grad.double(), p64.grad, rtol=1e-4, atol=1e-4 * float(p64.grad.abs().max()))
    assert float(p64.grad.abs().sum()) > 0
