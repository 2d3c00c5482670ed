"""-m gpu: CachedSDF / ComposedSDF / RobotSDF.ray_cast (csrc/ray_cast.hip) against the contract of include/pvamd.h "Ray casting":
the step loop restated HERE in torch around the existing point queries -- every step queries all the rays, torch.where freezes the
finished ones, a composition of A configurations is A one-configuration compositions of rows s * A + a -- and compared bit for
bit: integer outputs equal, float outputs the same bit patterns (NaN matching NaN), no ray left out.  Then the edges (partial
waves, the <= of the hit test, t_min > t_max, no rays), broadcasting, reproducibility, graph capture, the generic path, two
sanity checks and the C ABI.

The scenes.  Point queries of a cached grid never return a NaN value for a NaN coordinate (the range test fails and the
bounding-box branch ignores the component), so the INVALID status is provoked by what produces it in use, a NaN record: every
cache here is W.build_c2_cache() / build_robot() with the value of voxel (1, 1, 1) -- free space in a corner of the padding --
set to NaN once, when the fixture is built.  t_max is 2 m by default: a ray that leaves the scene doubles t every step and never
passes t_max = inf, so MISS needs a finite one."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from tests.helpers import GRID_Y_MAX
from tests.test_interp_gpu import build_robot
from tests.test_min_over_points_gpu import same_bits

pytestmark = pytest.mark.gpu

H_IMG, W_IMG = 36, 48
T_MAX = 2.0


# ---------------------------------------------------------------- the reference: the loop, in torch, around sdf(points)
def ref_loop(sdf, o, d, t_min=0.0, t_max=T_MAX, hit_tolerance=1e-3, step_scale=1.0, max_steps=128):
    """(t, status, values, gradients, steps) of (R, 3) rays; sdf(points) -> ((R,), (R, 3)).  Scalars are rounded once to the rays'
    dtype; o + t * d and t + step_scale * v are torch's eager elementwise kernels (a product, then a sum)."""
    R, T, dev = o.shape[0], o.dtype, o.device
    t_max, eps, scale = (torch.tensor(x, dtype=T, device=dev) for x in (t_max, hit_tolerance, step_scale))
    t = torch.full((R,), t_min, dtype=T, device=dev)
    t_read = t.clone()
    v = torch.full((R,), math.nan, dtype=T, device=dev)
    g = torch.full((R, 3), math.nan, dtype=T, device=dev)
    steps = torch.zeros(R, dtype=torch.int32, device=dev)
    status = torch.full((R,), pv.RAY_MAX_STEPS, dtype=torch.uint8, device=dev)
    active = t <= t_max
    status[~active] = pv.RAY_MISS
    for _ in range(max_steps):
        if not bool(active.any()):
            break
        p = o + t.unsqueeze(-1) * d
        vv, gg = sdf(p)
        vv, gg = vv.reshape(R), gg.reshape(R, 3)
        assert vv.dtype == T
        v = torch.where(active, vv, v)
        g = torch.where(active.unsqueeze(-1), gg, g)
        t_read = torch.where(active, t, t_read)
        steps = steps + active.int()
        invalid = active & (vv != vv)
        status[invalid] = pv.RAY_INVALID
        active = active & ~invalid
        hit = active & (vv <= eps)
        status[hit] = pv.RAY_HIT
        active = active & ~hit
        tn = t + scale * vv
        miss = active & ~(tn <= t_max)
        status[miss] = pv.RAY_MISS
        active = active & ~miss
        t = torch.where(active, tn, t)
    return t_read, status, v, g, steps


def configurations(sdf):
    """The callables the loop runs over: the SDF itself, or one single-configuration composition per configuration a, from rows
    s * A + a of the stack.  Returns (list, batch shape)."""
    comp = sdf.sdf if isinstance(sdf, pv.RobotSDF) else sdf
    if not isinstance(comp, pv.ComposedSDF):
        return [comp], ()
    batch = tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()
    S, A = len(comp.sdfs), math.prod(batch)
    stack = comp._tf_matrix.detach().reshape(S, A, 4, 4)
    ones = []
    for a in range(A):
        one = pv.ComposedSDF(comp.sdfs, None)
        one.set_transforms(stack[:, a].contiguous())
        ones.append(one)
    return ones, batch


_REF = {}


def reference(key, sdf, o, d, **kw):
    """The reference of a scene, computed once per (scene, dtype, arguments) and shared, as host arrays of shape B + (R,)."""
    key = (key, o.dtype, o.shape[0], tuple(sorted(kw.items())))
    if key not in _REF:
        ones, batch = configurations(sdf)
        with torch.no_grad():
            rows = [ref_loop(one, o, d, **kw) for one in ones]
        _REF[key] = tuple(torch.stack(x).reshape(*batch, *x[0].shape).cpu().numpy() for x in zip(*rows))
    return _REF[key]


def check(res, ref):
    assert isinstance(res, pv.RayCast)
    t, status, v, g, steps = ref
    assert res.status.dtype == torch.uint8 and res.steps.dtype == torch.int32
    assert res.t.dtype == res.values.dtype == res.gradients.dtype == torch.from_numpy(t).dtype
    assert res.status.shape == status.shape and np.array_equal(res.status.cpu().numpy(), status), "status"
    assert res.steps.shape == steps.shape and np.array_equal(res.steps.cpu().numpy(), steps), "steps"
    assert same_bits(res.t.cpu().numpy(), t), "t"
    assert same_bits(res.values.cpu().numpy(), v), "values"
    assert same_bits(res.gradients.cpu().numpy(), g), "gradients"


def statuses(ref):
    return {int(s) for s in np.unique(ref[1])}


# ---------------------------------------------------------------- scenes and rays
def poison(cache):
    """NaN into the value of voxel (1, 1, 1); returns that voxel's centre (leaf frame, float64)."""
    v = cache._view
    k = (1 * v.shape[1] + 1) * v.shape[2] + 1
    with torch.no_grad():
        cache._packed[k, 0] = math.nan
    return np.array([float(v.dmin[d]) + float(v.dres[d]) for d in range(3)])


def voxel_centre(cache, ijk):
    v = cache._view
    return np.array([float(v.dmin[d]) + ijk[d] * float(v.dres[d]) for d in range(3)])


def to_object(comp, s, a, x):
    """The object-frame point that transform (s, a) of a composition takes to the leaf-frame point x."""
    if comp is None:
        return np.asarray(x, np.float64)
    batch = tuple(comp.tsf_batch) if comp.tsf_batch is not None else ()
    M = comp._tf_matrix.detach().reshape(len(comp.sdfs), math.prod(batch), 4, 4)[s, a].double().cpu().numpy()
    return M[:3, :3].T @ (np.asarray(x, np.float64) - M[:3, 3])


def ray_set(leaf, comp, target, eye):
    """48 x 36 pinhole rays from `eye` towards `target` (half-angles atan 0.75 / atan 0.5625: the corner rays miss the padded
    grids entirely), float64 on the host, with the first rays replaced by the special ones.  `leaf` is the cache of leaf 0, whose
    frame the special origins are chosen in; `comp` (or None) takes them to the object frame under configuration 0."""
    target, eye = np.asarray(target, np.float64), np.asarray(eye, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    xs = np.linspace(-0.75, 0.75, W_IMG)
    ys = np.linspace(-0.5625, 0.5625, H_IMG)
    d = f[None, None] + xs[None, :, None] * r[None, None] + ys[:, None, None] * u[None, None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    o = np.broadcast_to(eye, d.shape).copy()
    values = torch.nan_to_num(leaf._packed[:, 0], nan=math.inf)  # (the NaN voxel is not the deepest one)
    deep = voxel_centre(leaf, np.unravel_index(int(torch.argmin(values)), tuple(leaf._view.shape)))
    res = float(leaf._view.dres[0])
    k = 0
    for j in range(5):  # inside the surface: HIT at step 1
        o[k] = to_object(comp, 0, 0, deep + 0.3 * res * np.array([(j & 1) - 0.5, ((j >> 1) & 1) - 0.5, (j >> 2) - 0.5]))
        k += 1
    centre = voxel_centre(leaf, [n // 2 for n in leaf._view.shape])
    for ijk in ((3, 3, 3), (4, 6, 3), (3, 5, 8), (6, 3, 4)):  # inside the grid's range, in the free space of the padding
        x = voxel_centre(leaf, ijk) + 0.2 * res
        o[k] = to_object(comp, 0, 0, x)
        aim = to_object(comp, 0, 0, centre) - o[k]
        d[k] = aim / np.linalg.norm(aim)
        k += 1
    o[k] = to_object(comp, 0, 0, voxel_centre(leaf, (1, 1, 1)))  # starts in the NaN voxel: INVALID at step 1
    k += 1
    o[k, 1] = math.nan  # a NaN origin component
    k += 1
    d[k] = 0.0  # a zero direction
    return torch.from_numpy(o), torch.from_numpy(d)


class Scene:
    def __init__(self, name, sdf, leaf, comp, target, eye):
        self.name, self.sdf = name, sdf
        self.o64, self.d64 = ray_set(leaf, comp, target, eye)

    def rays(self, dtype, R=None):
        o, d = self.o64.to(dtype).cuda(), self.d64.to(dtype).cuda()
        return (o, d) if R is None else (o[:R].contiguous(), d[:R].contiguous())


def grid_centre(cache):
    return np.array([(r[0] + r[1]) / 2 for r in cache.ranges], np.float64)


@pytest.fixture(scope="module")
def caches():
    out = {}
    for mode in ("nearest", "trilinear"):
        c = W.build_c2_cache()
        c.interpolation = mode
        poison(c)
        out[mode] = c
    return out


@pytest.fixture(scope="module")
def robots():
    out = {}
    for mode in ("nearest", "trilinear"):
        r = build_robot(interpolation=mode)
        r.set_joint_configuration(W.c4_joint_configs(3, seed=7).cuda())
        poison(r.sdf.sdfs[0])
        out[mode] = r
    return out


@pytest.fixture(scope="module")
def scenes(caches, robots):
    out = {}
    for mode in ("nearest", "trilinear"):
        c = caches[mode]
        centre = grid_centre(c)
        out["cached", mode] = Scene(f"cached-{mode}", c, c, None, centre, centre + [0.55, 0.2, 0.12])
        for A in (1, 3):
            comp = pv.ComposedSDF([c, c], None)
            comp.set_transforms(W.random_rigid(2 * A, seed=20 + A, trans=0.2).cuda(), batch_dim=(A,))
            out[f"composed{A}", mode] = Scene(f"composed{A}-{mode}", comp, c, comp, [0.0, 0.0, 0.0], [0.5, 0.3, 0.15])
        r = robots[mode]
        out["robot", mode] = Scene(f"robot-{mode}", r, r.sdf.sdfs[0], r.sdf, [0.0, 0.0, 0.45], [0.55, 0.2, 0.6])
    return out


KINDS = ["cached", "composed1", "composed3", "robot"]
MODES = ["nearest", "trilinear"]
DTYPES = [torch.float32, torch.float64]


# ---------------------------------------------------------------- bit for bit at R = 1728
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_full_fan(scenes, kind, mode, dtype):
    sc = scenes[kind, mode]
    o, d = sc.rays(dtype)
    assert o.shape == (H_IMG * W_IMG, 3)
    ref = reference(sc.name, sc.sdf, o, d)
    # conditions on the INPUTS: the reference alone must show every way a ray can end
    assert {pv.RAY_MISS, pv.RAY_HIT, pv.RAY_INVALID} <= statuses(ref), statuses(ref)
    assert int((ref[4][ref[1] == pv.RAY_HIT] == 1).sum()) >= 5  # the rays that start inside
    ref2 = reference(sc.name, sc.sdf, o, d, max_steps=2)
    assert pv.RAY_MAX_STEPS in statuses(ref2), statuses(ref2)
    check(sc.sdf.ray_cast(o, d, t_max=T_MAX), ref)
    check(sc.sdf.ray_cast(o, d, t_max=T_MAX, max_steps=2), ref2)
    if kind != "cached":  # ... and it was the kernel that answered
        assert (sc.sdf.sdf if kind == "robot" else sc.sdf)._fused_mode() == mode


# ---------------------------------------------------------------- more configurations than gridDim.y holds
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
def test_more_configurations_than_grid_rows(caches, mode, dtype):
    """composed_ray_cast_kernel wraps a += gridDim.y: configurations 65535.. are a block's second turn.  The loop restated above
    is one Python loop of up to 128 eager steps per configuration, far too slow for 65,601 of them, so it answers for the rows on
    either side of the wrap and a sample of the others; EVERY configuration is compared with the same call over two halves of the
    stack, neither of which wraps."""
    A = GRID_Y_MAX + 66
    edge = [0, 1, GRID_Y_MAX - 1, GRID_Y_MAX, GRID_Y_MAX + 1, A - 1]
    c = caches[mode]
    stack = W.random_rigid(2 * A, seed=31, trans=0.2).reshape(2, A, 4, 4)

    def composition(rows):
        comp = pv.ComposedSDF([c, c], None)
        part = stack[:, rows]
        comp.set_transforms(part.reshape(-1, 4, 4).cuda(), batch_dim=(part.shape[1],))
        return comp

    eye = np.array([0.5, 0.3, 0.15])
    aims = np.array([[0.0, 0.0, 0.0], [0.1, -0.1, 0.1], [1.0, 0.6, 0.3]]) - eye  # two towards the leaves, one away from them
    o = torch.from_numpy(np.broadcast_to(eye, (3, 3)).copy()).to(dtype).cuda()
    d = torch.from_numpy(aims / np.linalg.norm(aims, axis=1, keepdims=True)).to(dtype).cuda()
    res = composition(slice(None)).ray_cast(o, d, t_max=T_MAX)
    assert res.t.shape == (A, 3) and res.gradients.shape == (A, 3, 3)
    status = res.status.cpu().numpy()
    assert (status == pv.RAY_HIT).sum() > 100 and (status == pv.RAY_MISS).sum() > 100
    half = A // 2
    parts = [composition(slice(0, half)).ray_cast(o, d, t_max=T_MAX), composition(slice(half, A)).ray_cast(o, d, t_max=T_MAX)]
    assert equal_results(res, pv.RayCast(*(torch.cat(xy) for xy in zip(*parts))))
    rows = edge + sorted(np.random.default_rng(5).choice(A, 18, replace=False).tolist())
    ref = reference(f"many-{mode}", composition(rows), o, d)
    assert {pv.RAY_MISS, pv.RAY_HIT} <= statuses(ref), statuses(ref)
    check(pv.RayCast(*(x[rows] for x in res)), ref)
    check(pv.RayCast(*(x[edge] for x in res)), tuple(x[:len(edge)] for x in ref))  # rows 0, 1, 65534, 65535, 65536 and A - 1


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
def test_partial_waves_and_workgroups(scenes, R):
    sc = scenes["cached", "nearest"]
    o, d = sc.rays(torch.float32, R)
    check(sc.sdf.ray_cast(o, d, t_max=T_MAX), reference(sc.name, sc.sdf, o, d))


@pytest.mark.parametrize("kind,mode", [("cached", "trilinear"), ("composed3", "nearest")])
def test_step_scale_and_finite_t_max(scenes, kind, mode):
    sc = scenes[kind, mode]
    o, d = sc.rays(torch.float32)
    half = reference(sc.name, sc.sdf, o, d, step_scale=0.5)
    check(sc.sdf.ray_cast(o, d, t_max=T_MAX, step_scale=0.5), half)
    full = reference(sc.name, sc.sdf, o, d)
    assert (half[4] > full[4]).any()  # smaller steps: more of them
    cut = reference(sc.name, sc.sdf, o, d, t_max=0.45)
    check(sc.sdf.ray_cast(o, d, t_max=0.45), cut)
    assert ((cut[1] == pv.RAY_MISS) & (full[1] == pv.RAY_HIT)).any()  # t_max cut rays short that would have hit


@pytest.mark.parametrize("kind", ["cached", "composed3"])
def test_t_min_above_t_max(scenes, kind):
    sc = scenes[kind, "nearest"]
    o, d = sc.rays(torch.float32)
    res = sc.sdf.ray_cast(o, d, t_min=1.5, t_max=1.0)
    assert int(res.steps.abs().max()) == 0 and bool((res.status == pv.RAY_MISS).all())
    assert bool((res.t == 1.5).all()) and bool(res.values.isnan().all()) and bool(res.gradients.isnan().all())
    check(res, reference(sc.name, sc.sdf, o, d, t_min=1.5, t_max=1.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind,mode", [("cached", "nearest"), ("cached", "trilinear"), ("composed3", "trilinear")])
def test_hit_test_is_less_or_equal(scenes, kind, mode, dtype):
    """eps = a value the reference observed at some ray's SECOND step: that ray must stop there as HIT."""
    sc = scenes[kind, mode]
    o, d = sc.rays(dtype)
    t, status, v, g, steps = reference(sc.name, sc.sdf, o, d, max_steps=2)
    pick = np.argwhere((steps == 2) & (status == pv.RAY_MAX_STEPS) & np.isfinite(v) & (v > 1e-3))
    assert len(pick) > 0
    where = tuple(pick[len(pick) // 2])
    eps = float(v[where])  # exact: a float32 / float64 value as a Python float
    res = sc.sdf.ray_cast(o, d, t_max=T_MAX, hit_tolerance=eps)
    assert int(res.status[where]) == pv.RAY_HIT and int(res.steps[where]) == 2
    assert float(res.values[where]) == eps
    check(res, reference(sc.name, sc.sdf, o, d, hit_tolerance=eps))


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("kind", ["cached", "composed3", "robot"])
def test_broadcasting_and_shapes(scenes, kind):
    sc = scenes[kind, "nearest"]
    o, d = sc.rays(torch.float32)
    eye = o[-1]  # (3,): the camera centre (the special rays are the first ones)
    dirs = d.reshape(H_IMG, W_IMG, 3)
    res = sc.sdf.ray_cast(eye, dirs, t_max=T_MAX)
    B = (3,) if kind != "cached" else ()
    assert res.t.shape == res.status.shape == res.values.shape == res.steps.shape == B + (H_IMG, W_IMG)
    assert res.gradients.shape == B + (H_IMG, W_IMG, 3)
    ref = reference(sc.name + "-eye", sc.sdf, eye.expand(H_IMG * W_IMG, 3).contiguous(), d)
    check(pv.RayCast(*(x.reshape(*B, H_IMG * W_IMG, *x.shape[len(B) + 2:]) for x in res)), ref)
    # (H, 1, 3) origins against (1, W, 3) directions; rays that require grad are detached
    res2 = sc.sdf.ray_cast(eye.expand(H_IMG, 1, 3).clone().requires_grad_(), dirs[:1], t_max=T_MAX)
    assert res2.t.shape == B + (H_IMG, W_IMG) and not any(x.requires_grad for x in res2)
    assert same_bits(res2.t[..., 0, :].cpu().numpy(), res.t[..., 0, :].cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["cached", "composed3", "robot"])
def test_zero_rays(scenes, kind, dtype):
    sc = scenes[kind, "nearest"]
    B = (3,) if kind != "cached" else ()
    res = sc.sdf.ray_cast(torch.empty(0, 3, dtype=dtype, device="cuda"), torch.empty(2, 0, 3, dtype=dtype, device="cuda"))
    assert res.t.shape == res.status.shape == res.values.shape == res.steps.shape == B + (2, 0)
    assert res.gradients.shape == B + (2, 0, 3)
    assert res.t.dtype == res.values.dtype == res.gradients.dtype == dtype
    assert res.status.dtype == torch.uint8 and res.steps.dtype == torch.int32


# ---------------------------------------------------------------- reproducibility, graph capture
def equal_results(a, b):
    return all(same_bits(x.cpu().numpy(), y.cpu().numpy()) if x.dtype.is_floating_point else torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,mode", [("cached", "nearest"), ("robot", "trilinear")])
def test_reproducible(scenes, kind, mode):
    sc = scenes[kind, mode]
    o, d = sc.rays(torch.float32)
    assert equal_results(sc.sdf.ray_cast(o, d, t_max=T_MAX), sc.sdf.ray_cast(o, d, t_max=T_MAX))


@pytest.mark.parametrize("kind,mode", [("cached", "trilinear"), ("robot", "nearest")])
def test_graph_capture_single_stream(scenes, kind, mode):
    sc = scenes[kind, mode]
    o, d = sc.rays(torch.float32)
    eager = sc.sdf.ray_cast(o, d, t_max=T_MAX)  # the warm-up: descriptors built
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = sc.sdf.ray_cast(o, d, t_max=T_MAX)
    g.replay()
    torch.cuda.synchronize()
    assert equal_results(eager, cap)


# ---------------------------------------------------------------- the generic path
def test_generic_sphere_and_mixed_leaves(scenes, caches):
    sphere = pv.SphereSDF(0.08)
    sc = scenes["composed3", "nearest"]
    for dtype in DTYPES:
        o, d = sc.rays(dtype)
        ref = reference("sphere", sphere, o, d)
        assert {pv.RAY_MISS, pv.RAY_HIT, pv.RAY_INVALID} <= statuses(ref)  # the NaN origin: |p| is NaN
        check(sphere.ray_cast(o, d, t_max=T_MAX), ref)
    mixed = pv.ComposedSDF([caches["nearest"], caches["trilinear"]], None)
    mixed.set_transforms(sc.sdf._tf_matrix, batch_dim=(3,))
    assert mixed._fused_mode() is None
    o, d = sc.rays(torch.float32)
    ref = reference("mixed", mixed, o, d)
    assert {pv.RAY_MISS, pv.RAY_HIT} <= statuses(ref)
    res = mixed.ray_cast(o, d, t_max=T_MAX)
    assert res.t.shape == (3, H_IMG * W_IMG)
    check(res, ref)
    # float16 rays: the generic path, in the dtype __call__ returns
    assert scenes["cached", "nearest"].sdf.ray_cast(o.half(), d.half(), t_max=T_MAX, max_steps=4).values.dtype == torch.float16


# ---------------------------------------------------------------- sanity (not bits)
def test_sphere_hit_distance():
    """Rays aimed at the centre of a sphere from |o| = 1: with unit steps the march lands at the analytic distance |o| - radius
    up to rounding, and stops at the first sample within hit_tolerance of the surface.  float64: the rounding of the dozen
    operations on values of order 1 is below 1e-14."""
    radius, tol = 0.25, 1e-3
    g = torch.Generator().manual_seed(0)
    o = torch.nn.functional.normalize(torch.randn(500, 3, generator=g, dtype=torch.float64), dim=-1).cuda()
    res = pv.SphereSDF(radius).ray_cast(o, -o, hit_tolerance=tol)
    assert bool((res.status == pv.RAY_HIT).all())
    assert float((res.t - (1.0 - radius)).abs().max()) <= tol + 1e-12


def test_trilinear_hits_sit_on_the_surface(scenes):
    tol = 1e-3
    sc = scenes["cached", "trilinear"]
    o, d = sc.rays(torch.float32)
    res = sc.sdf.ray_cast(o, d, t_max=T_MAX, hit_tolerance=tol)
    on = (res.status == pv.RAY_HIT) & (res.steps > 1)
    assert int(on.sum()) > 20
    print("max |value| on HIT rays with steps > 1:", float(res.values[on].abs().max()))
    assert float(res.values[on].abs().max()) <= tol


# ---------------------------------------------------------------- C ABI
def abi_buffers(A, R, fill=None):
    make = (lambda s, dt: torch.empty(s, dtype=dt, device="cuda")) if fill is None else \
        (lambda s, dt: torch.full(s, fill, dtype=dt, device="cuda"))
    return (make((A, R), torch.float32), make((A, R), torch.uint8), make((A, R), torch.float32), make((A, R, 3), torch.float32),
            make((A, R), torch.int32))


def test_c_abi_call_equals_python(scenes):
    sc = scenes["composed3", "trilinear"]
    comp = sc.sdf
    o, d = sc.rays(torch.float32)
    want = comp.ray_cast(o, d, t_max=T_MAX)
    R = o.shape[0]
    dev = o.device
    grids, tfd = comp._leaf_grids(dev), comp._tf_device(dev)
    out = abi_buffers(3, R)
    rc = _lib.load().pvamd_composed_ray_cast(_lib.ptr(grids), 2, _lib.ptr(tfd), 3, _lib.ptr(o), _lib.ptr(d), R,
                                             _lib.LEAF_MODES["trilinear"], 0.0, T_MAX, 1e-3, 1.0, 128, *map(_lib.ptr, out),
                                             _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert equal_results(want, out)


def test_c_abi_bad_arguments_return_before_any_launch(scenes):
    sc = scenes["composed3", "nearest"]
    comp = sc.sdf
    o, d = sc.rays(torch.float32, 64)
    dev = o.device
    grids, tfd = comp._leaf_grids(dev), comp._tf_device(dev)
    lib = _lib.load()
    out = abi_buffers(3, 64, fill=77)
    desc = scenes["cached", "nearest"].sdf._grid_desc()

    def composed_call(t_max=T_MAX, eps=1e-3, scale=1.0, max_steps=128, outs=out):
        return lib.pvamd_composed_ray_cast(_lib.ptr(grids), 2, _lib.ptr(tfd), 3, _lib.ptr(o), _lib.ptr(d), 64, 0, 0.0, t_max, eps,
                                           scale, max_steps, *map(_lib.ptr, outs), _lib.stream_ptr())

    def cached_call(t_max=T_MAX, eps=1e-3, scale=1.0, max_steps=128, outs=out):
        return lib.pvamd_cached_ray_cast(ctypes.byref(desc), 0, _lib.ptr(o), _lib.ptr(d), 64, 0.0, t_max, eps, scale, max_steps,
                                         *map(_lib.ptr, outs), _lib.stream_ptr())

    for call in (composed_call, cached_call):
        assert call(max_steps=0) != 0 and call(max_steps=65536) != 0
        assert call(t_max=math.nan) != 0
        assert call(eps=-1e-6) != 0 and call(eps=math.inf) != 0
        assert call(scale=0.0) != 0
        for k in range(5):
            assert call(outs=tuple(None if j == k else x for j, x in enumerate(out))) != 0
    torch.cuda.synchronize()
    for x in out:  # nothing was launched: the buffers hold what they held
        assert bool((x == 77).all())
    # ... and zero rays / zero configurations are successful no-ops, whatever the pointers
    nothing = (None,) * 5
    assert lib.pvamd_composed_ray_cast(_lib.ptr(grids), 2, _lib.ptr(tfd), 3, None, None, 0, 0, 0.0, T_MAX, 1e-3, 1.0, 128,
                                       *map(_lib.ptr, nothing), _lib.stream_ptr()) == 0
    assert lib.pvamd_composed_ray_cast(_lib.ptr(grids), 2, _lib.ptr(tfd), 0, _lib.ptr(o), _lib.ptr(d), 64, 0, 0.0, T_MAX, 1e-3,
                                       1.0, 128, *map(_lib.ptr, nothing), _lib.stream_ptr()) == 0
    assert lib.pvamd_cached_ray_cast(ctypes.byref(desc), 0, None, None, 0, 0.0, T_MAX, 1e-3, 1.0, 128, *map(_lib.ptr, nothing),
                                     _lib.stream_ptr()) == 0
    assert cached_call() == 0  # the same call with good arguments runs
    torch.cuda.synchronize()
    assert not bool((out[4] == 77).all())
