"""-m gpu: ray_cast(..., differentiable=True) on the fused paths (csrc/ray_cast_backward.hip) against the float64 restatement of
include/pvamd.h "Ray casting: gradient of the hit distance" in tests/ray_backward_ref.py, within its bound
|got - ref| <= ulp_T(ref) / 2 + 8 N 2^-52 sum|term| (one float64 ulp first for float64), rows without a contributing pair exactly zero.

The scenes are built here: ~21^3-voxel caches (0.03 m, 0.1 m of padding) of mesh_io.box_mesh (half extents 0.2) and of
mesh_io.uv_sphere_mesh (radius 0.2), which take milliseconds.  The cached scenes carry a NaN record in voxel (1, 1, 1) -- free space
in a corner of the padding -- for the INVALID status, as tests/test_ray_cast_gpu.py does.  t_max is 2 m: a ray that leaves the
scene never passes t_max = inf."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib, mesh_io
from tests import ray_backward_ref as RB
from tests.helpers import STREAM_GRID_ITEMS
from tests.test_min_over_points_gpu import same_bits

pytestmark = pytest.mark.gpu

T_MAX = 2.0
KW = dict(t_max=T_MAX)
MODES = ["nearest", "trilinear"]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
CHUNK = _lib.RAY_BACKWARD_CHUNK


def build_cache(mesh, mode, poisoned):
    obj = pv.MeshObjectFactory(mesh=mesh)
    c = pv.CachedSDF("shape", 0.03, obj.bounding_box(padding=0.1), pv.MeshSDF(obj), device="cuda", cache_path=None,
                     interpolation=mode)
    assert all(18 <= n <= 24 for n in c._view.shape)
    if poisoned:
        v = c._view
        with torch.no_grad():
            c._packed[(1 * v.shape[1] + 1) * v.shape[2] + 1, 0] = math.nan
    return c


@pytest.fixture(scope="module")
def boxes():
    """The box cache with the NaN record, per interpolation."""
    return {mode: build_cache(mesh_io.box_mesh((0.2, 0.2, 0.2)), mode, True) for mode in MODES}


@pytest.fixture(scope="module")
def leaves():
    """The three leaves of the compositions, per interpolation: a box and two spheres, no NaN record."""
    return {mode: [build_cache(mesh_io.box_mesh((0.2, 0.2, 0.2)), mode, False),
                   build_cache(mesh_io.uv_sphere_mesh(0.2, 16, 8), mode, False),
                   build_cache(mesh_io.uv_sphere_mesh(0.2, 16, 8), mode, False)] for mode in MODES}


def voxel_centre(cache, ijk):
    v = cache._view
    return np.array([float(v.dmin[k]) + ijk[k] * float(v.dres[k]) for k in range(3)])


def fan(R, seed, radius, spread):
    """R rays from random origins on a sphere of `radius` towards random targets in the cube of half width `spread` (float64)."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(R, 3))
    o = radius * o / np.linalg.norm(o, axis=-1, keepdims=True)
    d = rng.uniform(-spread, spread, size=(R, 3)) - o
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def cached_rays(cache, R, dtype):
    """A fan at the box; from R = 64 on the first rays are: a central hit, a start in the NaN voxel (INVALID), a start inside the
    box pointing outward (a hit at t = 0 whose normal does not face the ray), a start inside pointing inward (a contributing hit at
    t = 0), a ray that passes the box by (MISS) and an oblique hit."""
    o, d = fan(R, 11, 0.6, 0.28)
    o[0], d[0] = (0.05, -0.02, 0.6), (0.0, 0.0, -1.0)
    if R >= 64:
        o[1] = voxel_centre(cache, (1, 1, 1))
        o[2], d[2] = (0.01, 0.02, 0.16), (0.0, 0.0, 1.0)
        o[3], d[3] = (0.05, 0.0, 0.16), (0.0, 0.0, -1.0)
        o[4], d[4] = (0.5, 0.5, 0.5), (1.0, 0.0, 0.0)
        aim = np.array([0.1, 0.0, 0.2]) - np.array([-0.5, 0.1, 0.5])
        o[5], d[5] = (-0.5, 0.1, 0.5), aim / np.linalg.norm(aim)
    return torch.from_numpy(o).to(dtype).cuda(), torch.from_numpy(d).to(dtype).cuda()


def weights(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) + 0.5).to(dtype).cuda()


def bits_equal(res, plain):
    """Every field: integer outputs equal, float outputs the same bit patterns (NaN matching NaN)."""
    for a, b in zip(res, plain):
        a, b = a.detach().cpu(), b.detach().cpu()
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        if not (same_bits(a.numpy(), b.numpy()) if a.dtype.is_floating_point else torch.equal(a, b)):
            return False
    return True


def only_t_carries_a_graph(res):
    return res.t.grad_fn is not None and all(x.grad_fn is None and not x.requires_grad for x in res[1:])


# ---------------------------------------------------------------- one cached grid
@DTYPES
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", [1, 64, 65, 257])
def test_cached(boxes, mode, dtype, R):
    cache = boxes[mode]
    o, d = cached_rays(cache, R, dtype)
    up = weights((R,), dtype, R)
    seen = set()
    for max_steps in (64, 2):
        plain = cache.ray_cast(o, d, max_steps=max_steps, **KW)
        og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
        res = cache.ray_cast(og, dg, max_steps=max_steps, differentiable=True, **KW)
        assert only_t_carries_a_graph(res) and bits_equal(res, plain)
        (res.t * up).sum().backward()
        terms = RB.pair_terms(o, d, plain.t, plain.status, plain.gradients, up)
        (ro, bo), (rd, bd) = RB.ray_reference(terms, dtype)
        RB.assert_within(og.grad, ro, bo, f"dorigins max_steps={max_steps}")
        RB.assert_within(dg.grad, rd, bd, f"ddirections max_steps={max_steps}")
        off = ~terms["on"]
        assert bool((og.grad.cpu()[off] == 0).all()) and bool((dg.grad.cpu()[off] == 0).all())
        assert og.grad.dtype == dtype and dg.grad.dtype == dtype and og.grad.shape == (R, 3)
        status = plain.status.cpu()
        seen |= {int(s) for s in status.unique()}
        if max_steps == 64:
            assert int(status[0]) == pv.RAY_HIT and bool(terms["on"][0])
            if R >= 64:
                assert status[:5].tolist() == [pv.RAY_HIT, pv.RAY_INVALID, pv.RAY_HIT, pv.RAY_HIT, pv.RAY_MISS]
                assert terms["on"][:5].tolist() == [True, False, False, True, False]  # ray 2: the normal faces away
                assert int(terms["on"].sum()) > R // 4
    if R >= 64:
        assert seen == {pv.RAY_MISS, pv.RAY_HIT, pv.RAY_MAX_STEPS, pv.RAY_INVALID}


@pytest.mark.parametrize("mode,dtype", [("nearest", torch.float32), ("trilinear", torch.float64)], ids=["nearest-f32", "trilinear-f64"])
def test_cached_with_more_rays_than_the_backward_grid_has_lanes(boxes, mode, dtype):
    """cached_ray_cast_backward_kernel runs on a capped streaming grid of kRayBwdBlock lanes per block: past that many rays a lane
    takes a second one.  The gradients of all the rays equal those of the same rays cast in two halves, neither of which
    strides, bit for bit (a ray's gradient depends on no other ray), and the 10,000 rays around the first stride stay within the
    bound of the float64 restatement."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(pv.__file__), "csrc", "ray_cast_backward.hip")).read()
    assert re.search(r"constexpr\s+int\s+kRayBwdBlock\s*=\s*PVAMD_RAY_BACKWARD_CHUNK\s*;", src)
    assert re.search(r"stream_grid\(R,\s*kRayBwdBlock\)", src)
    first = STREAM_GRID_ITEMS // 256 * CHUNK  # rays the capped grid covers in one turn
    R = first + 4099
    cache = boxes[mode]
    o, d = cached_rays(cache, R, dtype)
    up = weights((R,), dtype, 77)

    def gradients(rows):
        og, dg = o[rows].clone().requires_grad_(), d[rows].clone().requires_grad_()
        res = cache.ray_cast(og, dg, differentiable=True, **KW)
        (res.t * up[rows]).sum().backward()
        return res, og.grad, dg.grad

    res, go, gd = gradients(slice(0, R))
    half = R // 2
    assert half < first
    (_, go_a, gd_a), (_, go_b, gd_b) = gradients(slice(0, half)), gradients(slice(half, R))
    assert same_bits(go.cpu().numpy(), torch.cat((go_a, go_b)).cpu().numpy())
    assert same_bits(gd.cpu().numpy(), torch.cat((gd_a, gd_b)).cpu().numpy())
    rows = slice(first - 5000, first + 5000)
    terms = RB.pair_terms(o[rows], d[rows], res.t[rows], res.status[rows], res.gradients[rows], up[rows])
    (ro, bo), (rd, bd) = RB.ray_reference(terms, dtype)
    RB.assert_within(go[rows], ro, bo, "dorigins")
    RB.assert_within(gd[rows], rd, bd, "ddirections")
    on = terms["on"]
    assert int(on[:5000].sum()) > 500 and int(on[5000:].sum()) > 400  # contributing rays on both sides of the stride
    assert bool((go[rows].cpu()[~on] == 0).all()) and bool((gd[rows].cpu()[~on] == 0).all())
    assert bool((go[first:].abs().sum(dim=-1) > 0).any())


def test_box_face(boxes):
    """Rays that hit the +z face of the box away from its edges, where the interpolated stored gradient is n = (0, 0, 1): then
    c = d_z, w = -up / d_z, so dorigins = (0, 0, -1 / d_z) up and ddirections = t dorigins."""
    cache = build_cache(mesh_io.box_mesh((0.2, 0.2, 0.2)), "trilinear", False)
    # The records over the face carry the rounding of the mesh query that filled the cache (|n - e_z| up to 1.2e-6 here): this
    # test's own cache gets exactly e_z there, so that the premise holds and the interpolation of equal records is exact.
    with torch.no_grad():
        rec = cache._packed[:, 1:4]
        near = (rec[:, 2] > 0.999) & (rec[:, :2].abs() < 1e-3).all(dim=-1)
        print("records set to e_z:", int(near.sum()), "largest deviation before:",
              (rec[near] - torch.tensor([0.0, 0.0, 1.0], device=rec.device)).abs().max().item())
        assert int(near.sum()) > 100
        cache._packed[near, 1:4] = torch.tensor([0.0, 0.0, 1.0], device=rec.device)
    g = np.linspace(-0.08, 0.08, 5)
    o = np.array([[x, y, 0.5] for x in g for y in g])
    d = np.array([[0.1 * y, -0.15 * x - 0.01, -1.0] for x in g for y in g])
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    up = weights((25,), torch.float64, 5)
    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = cache.ray_cast(og, dg, hit_tolerance=1e-4, differentiable=True, **KW)
    assert bool((res.status == pv.RAY_HIT).all())
    n = res.gradients.cpu()
    print("largest |n - (0, 0, 1)|:", (n - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).abs().max().item())
    assert torch.equal(n, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(25, 3)), "the scene's premise: n = (0, 0, 1)"
    (res.t * up).sum().backward()
    t, d64, up64 = res.t.detach().cpu(), d.cpu(), up.cpu()
    want_o = torch.zeros(25, 3, dtype=torch.float64)
    want_o[:, 2] = -up64 / d64[:, 2]
    want_d = t.unsqueeze(-1) * want_o
    one = torch.ones(25, 1, dtype=torch.int64)
    RB.assert_within(og.grad, want_o, RB.bound(want_o, one, want_o.abs(), torch.float64), "dorigins")
    RB.assert_within(dg.grad, want_d, RB.bound(want_d, one, want_d.abs(), torch.float64), "ddirections")
    assert bool((og.grad[:, :2] == 0).all()) and bool((dg.grad[:, :2] == 0).all())


# ---------------------------------------------------------------- a composition
def composition(leaves, A, dtype, seed, grad=True):
    """S = 3: the box and a sphere near the origin, the second sphere at (5, 5, 5) where no ray reaches it."""
    S = len(leaves)
    m = W.random_rigid(S * A, seed=seed, trans=0.15).to(torch.float64)
    far = torch.tensor([5.0, 5.0, 5.0], dtype=torch.float64)
    for a in range(A):
        row = 2 * A + a
        m[row, :3, 3] = -(m[row, :3, :3] @ far)
    m = m.float().to(dtype).cuda().requires_grad_(grad)  # float64: the exact widening of a float32 stack
    comp = pv.ComposedSDF(list(leaves), None)
    comp.set_transforms(m, batch_dim=(A,))
    return comp, m


def composed_rays(R, dtype):
    """A fan at the two near leaves (the wide spread lets part of it miss); ray 1 is one that every configuration misses."""
    o, d = fan(R, 23, 0.8, 0.4)
    o[1], d[1] = (2.0, 2.0, 2.0), (-1.0, 0.0, 0.0)
    return torch.from_numpy(o).to(dtype).cuda(), torch.from_numpy(d).to(dtype).cuda()


def check_composed(comp, m, mode, dtype, A, R):
    S = len(comp.sdfs)
    assert comp._fused_mode() == mode
    o, d = composed_rays(R, dtype)
    up = weights((A, R), dtype, 100 * A + R)
    plain = comp.ray_cast(o, d, **KW)
    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = comp.ray_cast(og, dg, differentiable=True, **KW)
    assert res.t.shape == (A, R) and only_t_carries_a_graph(res) and bits_equal(res, plain)
    m.grad = None
    (res.t * up).sum().backward()
    assert m.grad.shape == (S * A, 4, 4) and m.grad.dtype == dtype and og.grad.dtype == dtype
    t, status, n = plain.t.reshape(A, R), plain.status.reshape(A, R), plain.gradients.reshape(A, R, 3)
    terms = RB.pair_terms(o, d, t, status, n, up)
    (ro, bo), (rd, bd) = RB.ray_reference(terms, dtype)
    RB.assert_within(og.grad, ro, bo, "dorigins")
    RB.assert_within(dg.grad, rd, bd, "ddirections")
    win = RB.winners(comp, o, d, t)
    rm, bm, count = RB.tf_reference(m.detach().reshape(S, A, 4, 4), win, terms, dtype)
    RB.assert_within(m.grad, rm, bm, "dtf")
    count = count.reshape(S, A)
    got = m.grad.cpu().reshape(S, A, 4, 4)
    assert int(count[0].sum()) > 0 and int(count[1].sum()) > 0 and int(count[2].sum()) == 0  # conditions on the scene
    assert bool((got[2] == 0).all()), "leaf 2 wins nowhere"
    assert bool((got[:, :, 3, :] == 0).all()), "bottom rows"
    assert bool((got[count == 0] == 0).all())
    assert bool((status[:, 1].cpu() == pv.RAY_MISS).all())
    none = ~terms["on"].any(dim=0)
    assert bool(none[1]) and bool((og.grad.cpu()[none] == 0).all()) and bool((dg.grad.cpu()[none] == 0).all())


@DTYPES
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("R", [65, CHUNK + 1])
def test_composed(leaves, mode, dtype, A, R):
    comp, m = composition(leaves[mode], A, dtype, seed=7 + A)
    check_composed(comp, m, mode, dtype, A, R)


def split_case():
    """The smallest shape whose plan puts two configurations into a split (include/pvamd.h item 4): 17 chunks want 121 splits."""
    R, A = 16 * CHUNK + 1, 122
    nchunks = -(-R // CHUNK)
    want = min(A, -(-2048 // nchunks))
    assert -(-A // want) == 2
    return A, R


def test_composed_more_configurations_than_splits(leaves):
    A, R = split_case()
    comp, m = composition(leaves["trilinear"], A, torch.float32, seed=31)
    check_composed(comp, m, "trilinear", torch.float32, A, R)


def test_generic_composition_rays(boxes):
    """A closed-form sphere next to a cache: no kernel serves it, the rays still get the contract's gradient (each
    configuration's term rounded to float32 by its own backward, then added by torch in float32: three roundings of at most
    2^-24 sum|term|)."""
    comp = pv.ComposedSDF([pv.SphereSDF(0.1), boxes["nearest"]], None)
    m = W.random_rigid(2 * 2, seed=3, trans=0.3).cuda()
    comp.set_transforms(m, batch_dim=(2,))
    assert comp._fused_mode() is None
    o, d = composed_rays(65, torch.float32)
    plain = comp.ray_cast(o, d, **KW)
    og = o.clone().requires_grad_()
    res = comp.ray_cast(og, d, differentiable=True, **KW)
    assert only_t_carries_a_graph(res) and bits_equal(res, plain)
    up = weights((2, 65), torch.float32, 9)
    (res.t * up).sum().backward()
    terms = RB.pair_terms(o, d, plain.t, plain.status, plain.gradients, up)
    assert int(terms["on"].sum()) > 10
    RB.assert_within(og.grad, terms["go"].sum(0), 3 * 2.0 ** -24 * terms["go"].abs().sum(0), "dorigins")
    m.requires_grad_()
    comp.set_transforms(m, batch_dim=(2,))
    with pytest.raises(ValueError, match="transforms"):
        comp.ray_cast(og, d, differentiable=True, **KW)


# ---------------------------------------------------------------- a robot
def test_robot_joint_gradient():
    """q.grad of res.t.sum() against the restated dtf pushed through the same configure path.  That path is linear in its
    upstream: dq = J^T dstack in float64, J = d stack / d q, rounded once to float32.  The kernel's dtf and the float32 rounding
    of the restated one differ by at most bound(dtf) + ulp(dtf) / 2, so
        |dq - dq_ref| <= |J|^T (bound(dtf) + ulp_f32(dtf_ref) / 2) + ulp_f32(dq_ref) + 2 K 2^-52 |J|^T |dtf_ref|
    with K = 12 S A products per joint value (the float64 contraction's own rounding on either side)."""
    robot = W.build_c4()
    A, H, Wd = 2, 16, 16
    q = W.c4_joint_configs(A, seed=3).cuda().requires_grad_()
    robot.set_joint_configuration(q)
    comp = robot.sdf
    S = len(comp.sdfs)
    stack = comp._tf_matrix
    assert stack.requires_grad and comp._fused_mode() == "nearest"
    stack.retain_grad()
    eye = torch.tensor([1.2, 0.5, 0.8])
    f = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 0.45]) - eye, dim=0)
    r = torch.nn.functional.normalize(torch.linalg.cross(f, torch.tensor([0.0, 0.0, 1.0])), dim=0)
    u = torch.linalg.cross(r, f)
    xs, ys = torch.linspace(-0.35, 0.35, Wd), torch.linspace(0.35, -0.35, H)
    dirs = torch.nn.functional.normalize(f + xs[None, :, None] * r + ys[:, None, None] * u, dim=-1).cuda()
    eye = eye.cuda()
    res = robot.ray_cast(eye, dirs, t_max=3.0, differentiable=True)
    assert res.t.shape == (A, H, Wd) and only_t_carries_a_graph(res)
    assert bits_equal(res, robot.ray_cast(eye, dirs, t_max=3.0))
    res.t.sum().backward()
    R = H * Wd
    o, d = eye.expand(R, 3).contiguous(), dirs.reshape(R, 3)
    t, status, n = res.t.detach().reshape(A, R), res.status.reshape(A, R), res.gradients.reshape(A, R, 3)
    terms = RB.pair_terms(o, d, t, status, n, torch.ones(A, R))
    assert int(terms["on"].sum()) > 20
    win = RB.winners(comp, o, d, t)
    rm, bm, _ = RB.tf_reference(stack.detach().reshape(S, A, 4, 4), win, terms, torch.float32)
    RB.assert_within(stack.grad, rm, bm, "dtf")
    q2 = q.detach().clone().requires_grad_()
    robot.set_joint_configuration(q2)
    (rm.to(device=q2.device, dtype=torch.float32) * robot.sdf._tf_matrix).sum().backward()
    J = torch.autograd.functional.jacobian(robot._stack_torch, q.detach().double()).abs().cpu()  # (S A, 4, 4, A, M)
    slack = bm + RB.ulp(rm, torch.float32) / 2
    tol = torch.einsum("sijam,sij->am", J, slack) + RB.ulp(RB.host64(q2.grad), torch.float32) + \
        2 * 12 * S * A * RB.EPS64 * torch.einsum("sijam,sij->am", J, rm.abs())
    RB.assert_within(q.grad, RB.host64(q2.grad), tol, "dq")
    assert float(q.grad.abs().max()) > 0


# ---------------------------------------------------------------- reproducible, capturable, inside its scratch
def backward_of(sdf, o, d, up, extra=()):
    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = sdf.ray_cast(og, dg, differentiable=True, **KW)
    return torch.autograd.grad((res.t * up).sum(), (og, dg) + tuple(extra))


def test_two_backward_calls_give_the_same_bits(boxes, leaves):
    A, R = 3, 1000
    comp, m = composition(leaves["trilinear"], A, torch.float32, seed=5)
    o, d = composed_rays(R, torch.float32)
    up = weights((A, R), torch.float32, 1)
    first, second = backward_of(comp, o, d, up, (m,)), backward_of(comp, o, d, up, (m,))
    assert all(torch.equal(x, y) for x, y in zip(first, second)) and float(first[2].abs().max()) > 0
    o, d = cached_rays(boxes["nearest"], R, torch.float64)
    up = weights((R,), torch.float64, 2)
    first, second = backward_of(boxes["nearest"], o, d, up), backward_of(boxes["nearest"], o, d, up)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


@pytest.mark.parametrize("kind", ["cached", "composed"])
def test_forward_and_backward_replay_from_a_graph(boxes, leaves, kind):
    """Capturing a backward follows torch's rule for it: every leaf that receives a gradient is made, and the warm-up run, on the
    stream the capture uses.  Autograd synchronises a gradient with the stream its leaf was made on, and a wait of another stream
    inside a capture forks it without a join."""
    A, R = 3, 700
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if kind == "cached":
            sdf, extra = boxes["trilinear"], ()
            o, d = cached_rays(sdf, R, torch.float32)
            up = weights((R,), torch.float32, 3)
        else:
            sdf, m = composition(leaves["nearest"], A, torch.float32, seed=6)
            extra = (m,)
            o, d = composed_rays(R, torch.float32)
            up = weights((A, R), torch.float32, 4)
        eager = backward_of(sdf, o, d, up, extra)  # the warm-up: descriptors built, the stack on the device
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        captured = backward_of(sdf, o, d, up, extra)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(eager, captured))
    assert float(eager[0].abs().max()) > 0


@DTYPES
@pytest.mark.parametrize("A,R", [(1, 1000), (3, CHUNK + 1), split_case()], ids=["no_split", "two_chunks", "two_per_split"])
def test_backward_stays_inside_its_scratch(leaves, monkeypatch, dtype, A, R):
    """In the style of tests/test_scratch_bounds_gpu.py: the scratch is handed out in front of a 1 MiB tail of 0xA5 that belongs
    to the test, so an overrun shows as a changed byte."""
    tail, fill, handed = 1 << 20, 0xA5, []

    def guarded(nbytes, dev):
        whole = torch.empty((nbytes + tail,), dtype=torch.uint8, device=dev)
        whole[nbytes:] = fill
        handed.append((whole, nbytes))
        return whole[:nbytes]

    comp, m = composition(leaves["nearest"], A, dtype, seed=A)
    o, d = composed_rays(R, dtype)
    monkeypatch.setattr(_lib, "scratch_buffer", guarded)
    backward_of(comp, o, d, weights((A, R), dtype, 8), (m,))
    torch.cuda.synchronize()
    assert len(handed) == 1
    whole, nbytes = handed[0]
    assert nbytes == max(_lib.ray_cast_backward_scratch_bytes(3, A, R, dtype == torch.float64), 16)
    assert bool((whole[nbytes:] == fill).all()), f"a kernel wrote past its {nbytes}-byte scratch"


# ---------------------------------------------------------------- the C ABI
def test_c_abi_bad_arguments_return_before_any_launch(boxes, leaves):
    lib = _lib.load()
    R, A, S = 64, 3, 3
    comp, m = composition(leaves["nearest"], A, torch.float32, seed=2, grad=False)
    o, d = composed_rays(R, torch.float32)
    dev = o.device
    plain = comp.ray_cast(o, d, **KW)
    grids, tfd = comp._leaf_grids(dev), comp._tf_device(dev)
    t, status, grad = plain.t.contiguous(), plain.status.contiguous(), plain.gradients.contiguous()
    up = torch.ones((A, R), device=dev)
    go, gd, gtf = (torch.full(shape, 77.0, device=dev) for shape in ((R, 3), (R, 3), (S * A, 4, 4)))
    scratch = _lib.scratch_buffer(_lib.ray_cast_backward_scratch_bytes(S, A, R, False), dev)
    good = dict(grids=grids, S=S, tf=tfd, A=A, o=o, d=d, R=R, mode=0, t=t, status=status, up=up, go=go, gd=gd, gtf=gtf,
                scratch=scratch)

    def addr(x, shift=0):
        return x if isinstance(x, int) else ctypes.c_void_p((x.data_ptr() + shift) if x is not None else 0)

    def composed_call(shift=None, **change):
        a = dict(good, **change)
        p = {k: addr(v, 1 if k == shift else 0) for k, v in a.items()}
        return lib.pvamd_composed_ray_cast_backward(p["grids"], a["S"], p["tf"], a["A"], p["o"], p["d"], a["R"], a["mode"], p["t"],
                                                    p["status"], p["up"], p["go"], p["gd"], p["gtf"], p["scratch"], _lib.stream_ptr())

    assert composed_call(S=0) == -2 and composed_call(S=65) == -2 and composed_call(A=-1) == -2 and composed_call(R=-1) == -2
    assert composed_call(mode=2) == -4 and composed_call(mode=-1) == -4
    for k in ("grids", "tf", "o", "d", "t", "status", "up", "scratch"):
        assert composed_call(**{k: None}) == -1, k
    for k in ("tf", "o", "d", "t", "up", "go", "gd", "gtf", "scratch"):
        assert composed_call(shift=k) == -3, k

    ct, cs, cg, cup = t[0].contiguous(), status[0].contiguous(), grad[0].contiguous(), up[0].contiguous()

    def cached_call(shift=None, R=R, **change):
        a = dict(dict(d=d, t=ct, status=cs, grad=cg, up=cup, go=go, gd=gd), **change)
        p = {k: addr(v, 1 if k == shift else 0) for k, v in a.items()}
        return lib.pvamd_cached_ray_cast_backward(p["d"], R, p["t"], p["status"], p["grad"], p["up"], p["go"], p["gd"],
                                                  _lib.stream_ptr())

    assert cached_call(R=-1) == -2
    for k in ("d", "t", "status", "grad", "up"):
        assert cached_call(**{k: None}) == -1, k
    for k in ("d", "t", "grad", "up", "go", "gd"):
        assert cached_call(shift=k) == -3, k
    torch.cuda.synchronize()
    for x in (go, gd, gtf):  # nothing was launched: the buffers hold what they held
        assert bool((x == 77.0).all())
    # nothing wanted, no rays: successful no-ops
    assert composed_call(go=None, gd=None, gtf=None) == 0 and cached_call(go=None, gd=None) == 0 and cached_call(R=0) == 0
    assert lib.pvamd_ray_cast_backward_scratch_bytes(0, A, R, 0) == 0
    # ... and the same calls with good arguments run, and give what the Python path gives
    assert composed_call() == 0 and not bool((gtf == 77.0).any())
    m2 = m.clone().requires_grad_()
    comp.set_transforms(m2, batch_dim=(A,))
    want = backward_of(comp, o, d, up, (m2,))
    torch.cuda.synchronize()
    assert torch.equal(go, want[0]) and torch.equal(gd, want[1]) and torch.equal(gtf, want[2])
    assert cached_call() == 0
