"""CPU: the ray_cast API surface (pv.RayCast, pv.RAY_*, CachedSDF / ComposedSDF / RobotSDF.ray_cast), its argument checks, the
ctypes mirrors of the four entry points, and the loop of include/pvamd.h "Ray casting" restated here in plain Python floats on a
closed-form sphere and checked on hand-computed rays, together with the torch loop of the generic path on the same rays.  No GPU:
every check here raises, or runs on CPU tensors, before a kernel could be launched."""
import math
import os
import re

import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import sdf as sdf_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pvamd_cached_ray_cast", "pvamd_cached_ray_cast_f64", "pvamd_composed_ray_cast", "pvamd_composed_ray_cast_f64")


def test_exports():
    assert pv.RayCast is sdf_mod.RayCast
    assert pv.RayCast._fields == ("t", "status", "values", "gradients", "steps")
    assert (pv.RAY_MISS, pv.RAY_HIT, pv.RAY_MAX_STEPS, pv.RAY_INVALID) == (0, 1, 2, 3)
    assert (_lib.RAY_MISS, _lib.RAY_HIT, _lib.RAY_MAX_STEPS, _lib.RAY_INVALID) == (0, 1, 2, 3)
    for cls in (pv.ObjectFrameSDF, pv.CachedSDF, pv.ComposedSDF, pv.RobotSDF):
        assert callable(cls.ray_cast)
    assert pv.CachedSDF.ray_cast is not pv.ObjectFrameSDF.ray_cast and pv.ComposedSDF.ray_cast is not pv.ObjectFrameSDF.ray_cast


def test_abi_mirrors_and_status_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "pvamd.h")).read()
    for name, code in (("MISS", 0), ("HIT", 1), ("MAX_STEPS", 2), ("INVALID", 3)):
        assert re.search(rf"#define\s+PVAMD_RAY_{name}\s+{code}\b", text), name
    assert re.search(r"#define\s+PVAMD_ABI_VERSION\s+16\b", text)
    assert _lib.ABI_VERSION == 16
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params) == (16 if "cached" in name else 19), name
        real = "double" if name.endswith("_f64") else "float"
        scalars = [p for p in params if "*" not in p]
        # R, the four reals in the entry point's element type, max_steps (and S, A, mode)
        assert sum(p.startswith(real + " ") for p in scalars) == 4, (name, scalars)
        import ctypes
        assert sum(a is (ctypes.c_double if real == "double" else ctypes.c_float) for a in argtypes) == 4, name
    assert os.path.exists(os.path.join(ROOT, "pytorch_volumetric_amd", "csrc", "ray_cast.hip"))


# ---------------------------------------------------------------- argument checks (nothing here reaches a device)
def sphere():
    return pv.SphereSDF(0.25)


def composed(with_transforms=True):
    c = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
    if with_transforms:
        m = torch.eye(4).repeat(2 * 3, 1, 1)
        m[:, 0, 3] = torch.arange(6.0) * 0.1
        c.set_transforms(m, batch_dim=(3,))
    return c


def planar_cache():
    """A CachedSDF cannot be built without a GPU; ray_cast must refuse a planar one before it looks at anything on a device."""
    c = object.__new__(pv.CachedSDF)
    object.__setattr__(c, "_dim", 2)
    return c


O, D = torch.zeros(4, 3), torch.tensor([0.0, 0.0, 1.0])
TARGETS = [sphere, composed, planar_cache]


@pytest.mark.parametrize("make", TARGETS)
def test_value_errors(make):
    s = make()
    bad_shapes = [(torch.zeros(4, 2), D), (O, torch.zeros(4)), (torch.tensor(1.0), D), (torch.zeros(4, 3), torch.zeros(5, 3)),
                  (torch.zeros(2, 4, 3), torch.zeros(3, 1, 3))]
    for o, d in bad_shapes:
        with pytest.raises(ValueError):
            s.ray_cast(o, d)
    for kw in ({"t_min": math.nan}, {"t_max": math.nan}, {"hit_tolerance": -1e-9}, {"hit_tolerance": math.inf},
               {"hit_tolerance": math.nan}, {"step_scale": 0.0}, {"step_scale": -0.5}, {"step_scale": math.inf},
               {"step_scale": math.nan}, {"max_steps": 0}, {"max_steps": -3}, {"max_steps": 65536}):
        with pytest.raises(ValueError):
            s.ray_cast(O, D, **kw)


@pytest.mark.parametrize("make", TARGETS)
def test_type_errors(make):
    s = make()
    for bad in (1.5, "8", None, True, 128.0):
        with pytest.raises(TypeError):
            s.ray_cast(O, D, max_steps=bad)


def test_transforms_must_be_set():
    with pytest.raises(ValueError):
        composed(with_transforms=False).ray_cast(O, D)


def test_planar_cache_raises():
    with pytest.raises(ValueError, match="planar"):
        planar_cache().ray_cast(O, D)


# ---------------------------------------------------------------- the loop, restated in Python floats (float64)
def restated(o, d, radius, t_min=0.0, t_max=math.inf, eps=1e-3, step_scale=1.0, max_steps=128):
    """include/pvamd.h "Ray casting" for one ray against the closed-form sphere |p| - radius.  Python floats are float64 and
    every operation below rounds on its own.  The reported t is that of the last evaluated point (output rule 3)."""
    t, steps, v = t_min, 0, math.nan
    if not (t <= t_max):
        return t, pv.RAY_MISS, steps, v
    for _ in range(max_steps):
        p = [o[j] + t * d[j] for j in range(3)]
        v = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) - radius
        t_read = t
        steps += 1
        if v != v:
            return t_read, pv.RAY_INVALID, steps, v
        if v <= eps:
            return t_read, pv.RAY_HIT, steps, v
        tn = t + step_scale * v
        if not (tn <= t_max):
            return t_read, pv.RAY_MISS, steps, v
        t = tn
    return t_read, pv.RAY_MAX_STEPS, steps, v


HAND = [
    # aimed at the centre from 1 m: the first sample reads 0.75, the second sits on the surface
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, 1.0)), (0.75, pv.RAY_HIT, 2)),
    # starting inside: a hit at the first sample, t stays t_min
    (dict(o=(0.0, 0.0, 0.0), d=(1.0, 0.0, 0.0)), (0.0, pv.RAY_HIT, 1)),
    # pointing away: the value grows, the second step would pass t_max = 2
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, -1.0), t_max=2.0), (0.75, pv.RAY_MISS, 2)),
    # t_min > t_max: nothing evaluated
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, 1.0), t_min=3.0, t_max=2.0), (3.0, pv.RAY_MISS, 0)),
    # half steps towards the centre: 0.75, 0.375, 0.1875, ... the value halves; it is <= 1e-3 at the 11th sample
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, 1.0), step_scale=0.5), (0.75 * (1 - 2.0 ** -10), pv.RAY_HIT, 11)),
    # ... and three samples are not enough
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, 1.0), step_scale=0.5, max_steps=3), (0.375 + 0.1875, pv.RAY_MAX_STEPS, 3)),
    # a zero direction never moves: value 0.75 at every sample, t grows by it
    (dict(o=(0.0, 0.0, -1.0), d=(0.0, 0.0, 0.0), max_steps=4), (2.25, pv.RAY_MAX_STEPS, 4)),
    # a NaN origin: invalid at the first sample
    (dict(o=(math.nan, 0.0, -1.0), d=(0.0, 0.0, 1.0)), (0.0, pv.RAY_INVALID, 1)),
]


@pytest.mark.parametrize("case,want", HAND)
def test_hand_computed_rays(case, want):
    t, status, steps, v = restated(radius=0.25, **case)
    assert (t, status, steps) == want
    # the generic path (the torch loop around SphereSDF.__call__) on the same ray, in float64: SphereSDF computes
    # linalg.norm - radius, which for these axis-aligned rays is exact like the restatement
    kw = {k: case[k] for k in ("t_min", "t_max", "step_scale", "max_steps") if k in case}
    r = sphere().ray_cast(torch.tensor(case["o"], dtype=torch.float64), torch.tensor(case["d"], dtype=torch.float64), **kw)
    assert isinstance(r, pv.RayCast)
    assert r.t.shape == () and r.gradients.shape == (3,)
    assert r.status.dtype == torch.uint8 and r.steps.dtype == torch.int32 and r.t.dtype == r.values.dtype == torch.float64
    assert (float(r.t), int(r.status), int(r.steps)) == want
    if steps == 0:
        assert math.isnan(float(r.values)) and bool(torch.isnan(r.gradients).all())
    elif status != pv.RAY_INVALID:
        assert float(r.values) == v


def test_generic_shapes_broadcast_empty_and_detach():
    s = sphere()
    o = torch.tensor([0.0, 0.0, -1.0], requires_grad=True)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.3, 1.0], [1.0, 0.0, 0.0]]).repeat(2, 1, 1), dim=-1)
    r = s.ray_cast(o, d, t_max=10.0)
    assert r.t.shape == r.status.shape == r.values.shape == r.steps.shape == (2, 3) and r.gradients.shape == (2, 3, 3)
    assert not any(x.requires_grad for x in r)
    assert r.status[0].tolist() == [pv.RAY_HIT, pv.RAY_MISS, pv.RAY_MISS]
    e = s.ray_cast(torch.empty(0, 3), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    assert e.t.shape == (0,) and e.gradients.shape == (0, 3) and e.t.dtype == torch.float64 and e.status.dtype == torch.uint8
    # integer rays count as float32, as integer points do
    i = s.ray_cast(torch.tensor([0, 0, -1]), torch.tensor([0, 0, 1]))
    assert i.t.dtype == torch.float32 and float(i.t) == 0.75 and int(i.status) == pv.RAY_HIT
