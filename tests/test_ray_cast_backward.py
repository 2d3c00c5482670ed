"""CPU: ray_cast(..., differentiable=True) -- the keyword on the four classes, the cases that keep today's path, and the generic
(torch) path of include/pvamd.h "Ray casting: gradient of the hit distance" on closed-form spheres, against the float64
restatement of tests/ray_backward_ref.py within its bound.  No GPU: everything here runs on CPU tensors."""
import inspect
import os
import re

import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import ray_backward_ref as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T64 = torch.float64


def sphere_rays():
    """SphereSDF(0.25) at the origin, five unit rays: a central hit, two oblique hits, a miss (finite t_max), and one that starts
    inside and points outward (a hit at t = 0 whose normal faces away from the ray)."""
    o = torch.tensor([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0], [0.0, -0.15, 1.0], [0.5, 0.0, 1.0], [0.0, 0.0, 0.1]], dtype=T64)
    d = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.2, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]], dtype=T64)
    d = d / d.norm(dim=-1, keepdim=True)
    return o, d


KW = dict(t_max=3.0, hit_tolerance=1e-6)


def test_signature_has_differentiable_last_on_all_four_classes():
    for cls in (pv.ObjectFrameSDF, pv.CachedSDF, pv.ComposedSDF, pv.RobotSDF):
        params = list(inspect.signature(cls.ray_cast).parameters.values())
        assert params[-1].name == "differentiable" and params[-1].default is False, cls.__name__
        assert [p.name for p in params[1:]] == ["origins", "directions", "t_min", "t_max", "hit_tolerance", "step_scale", "max_steps",
                                                "differentiable"], cls.__name__
    assert pv.RayCast._fields == ("t", "status", "values", "gradients", "steps")
    o, d = sphere_rays()
    res = pv.SphereSDF(0.25).ray_cast(o, d, differentiable=False, **KW)
    assert res.t.grad_fn is None


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, torch.tensor(True)])
def test_a_non_bool_raises_type_error(bad):
    o, d = sphere_rays()
    comp = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
    comp.set_transforms(torch.eye(4).repeat(2, 1, 1))
    for sdf in (pv.SphereSDF(0.25), comp):
        with pytest.raises(TypeError):
            sdf.ray_cast(o, d, differentiable=bad)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))


def test_nothing_to_differentiate_keeps_todays_path():
    o, d = sphere_rays()
    s = pv.SphereSDF(0.25)
    plain = s.ray_cast(o, d, **KW)
    res = s.ray_cast(o, d, differentiable=True, **KW)  # nothing requires grad
    with torch.no_grad():
        quiet = s.ray_cast(o.clone().requires_grad_(), d, differentiable=True, **KW)
    off = s.ray_cast(o.clone().requires_grad_(), d, **KW)  # requires grad, not asked for: detached, as before
    for r in (res, quiet, off):
        assert all(x.grad_fn is None and not x.requires_grad for x in r)
        assert all(same(x, y) for x, y in zip(r, plain))


def test_sphere_gradients_match_the_restatement():
    o, d = sphere_rays()
    s = pv.SphereSDF(0.25)
    plain = s.ray_cast(o, d, **KW)
    assert plain.status.tolist() == [pv.RAY_HIT, pv.RAY_HIT, pv.RAY_HIT, pv.RAY_MISS, pv.RAY_HIT]
    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res = s.ray_cast(og, dg, differentiable=True, **KW)
    assert res.t.grad_fn is not None and res.t.requires_grad
    assert all(x.grad_fn is None and not x.requires_grad for x in res[1:])
    assert all(same(x, y) for x, y in zip(res, plain)), "the forward's bits"
    up = torch.tensor([1.0, -0.75, 2.5, 1.25, 0.5], dtype=T64)
    (res.t * up).sum().backward()
    terms = RB.pair_terms(o, d, plain.t, plain.status, plain.gradients, up)
    assert terms["on"].tolist() == [True, True, True, False, False]
    (ro, bo), (rd, bd) = RB.ray_reference(terms, T64)
    RB.assert_within(og.grad, ro, bo, "dorigins")
    RB.assert_within(dg.grad, rd, bd, "ddirections")
    # the central ray: dt/do = -d (n = -d there, c = -1)
    RB.assert_within(og.grad[0], -d[0] * up[0], bo[0], "central ray")
    for i in (3, 4):  # the miss and the outward-facing hit
        assert torch.equal(og.grad[i], torch.zeros(3, dtype=T64)) and torch.equal(dg.grad[i], torch.zeros(3, dtype=T64))
    assert og.grad.dtype == T64 and dg.grad.dtype == T64


def test_a_shared_origin_gets_the_sum():
    _, d = sphere_rays()
    d = d[:3]
    eye = torch.tensor([0.02, -0.01, 1.0], dtype=T64)
    s = pv.SphereSDF(0.25)
    e = eye.clone().requires_grad_()
    res = s.ray_cast(e, d, differentiable=True, **KW)
    assert res.t.shape == (3,) and (res.status == pv.RAY_HIT).all()
    res.t.sum().backward()
    per_ray = eye.expand(3, 3).clone().requires_grad_()
    s.ray_cast(per_ray, d, differentiable=True, **KW).t.sum().backward()
    assert e.grad.shape == (3,)
    assert torch.equal(e.grad, per_ray.grad.sum(0))
    # one float32 side promotes: the gradient comes back in the input's own dtype
    e32 = eye.float().requires_grad_()
    s.ray_cast(e32, d, differentiable=True, **KW).t.sum().backward()
    assert e32.grad.dtype == torch.float32 and torch.allclose(e32.grad.double(), e.grad, rtol=1e-5, atol=1e-6)


def generic_composition(requires_grad):
    comp = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
    m = torch.eye(4).repeat(2 * 2, 1, 1)  # leaf-major: (leaf 0: a = 0, 1), (leaf 1: a = 0, 1)
    m[:, 0, 3] = torch.tensor([0.3, 0.35, -0.3, -0.25])
    if requires_grad:
        m.requires_grad_()
    comp.set_transforms(m, batch_dim=(2,))
    return comp, m


def test_generic_composition_with_transforms_that_require_grad_raises():
    """A composition of closed-form spheres is served by no kernel: its transforms would get no gradient, so the call refuses --
    before it touches a device -- when they require grad, whether or not the rays do.  (Its __call__ needs the device, so the
    rays' gradients of this composition are checked in test_ray_cast_backward_gpu.py.)"""
    o = torch.tensor([[-0.3, 0.0, 1.0], [0.3, 0.02, 1.0], [0.0, 0.0, 1.0]])
    d = torch.tensor([0.0, 0.0, -1.0])
    comp, m = generic_composition(True)
    assert comp._fused_mode() is None and comp._tf_grad
    with pytest.raises(ValueError, match="transforms"):
        comp.ray_cast(o, d, differentiable=True, **KW)
    with pytest.raises(ValueError, match="transforms"):
        comp.ray_cast(o.clone().requires_grad_(), d, differentiable=True, **KW)
    with pytest.raises(TypeError):
        comp.ray_cast(o, d, differentiable=1, **KW)


def test_double_backward_raises():
    o, d = sphere_rays()
    og = o.clone().requires_grad_()
    res = pv.SphereSDF(0.25).ray_cast(og, d, differentiable=True, **KW)
    with pytest.raises(RuntimeError):
        (g,) = torch.autograd.grad(res.t.sum(), og, create_graph=True)
        g.sum().backward()


def test_mutating_a_saved_input_raises():
    o, d = sphere_rays()
    og = o.clone().requires_grad_()
    dd = d.clone()
    res = pv.SphereSDF(0.25).ray_cast(og, dd, differentiable=True, **KW)
    dd.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        res.t.sum().backward()


SYMBOLS = {"pvamd_cached_ray_cast_backward": 9, "pvamd_cached_ray_cast_backward_f64": 9, "pvamd_composed_ray_cast_backward": 16,
           "pvamd_composed_ray_cast_backward_f64": 16}


def test_abi_mirrors_match_the_header():
    text = open(os.path.join(ROOT, "include", "pvamd.h")).read()
    assert "Ray casting: gradient of the hit distance" in text
    assert text.index("Ray casting: gradient of the hit distance") > text.index("---- Ray casting (")
    assert re.search(r"#define\s+PVAMD_ABI_VERSION\s+16\b", text) and _lib.ABI_VERSION == 16
    assert re.search(rf"#define\s+PVAMD_RAY_BACKWARD_CHUNK\s+{_lib.RAY_BACKWARD_CHUNK}\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert not re.search(r"#define\s+PVAMD_RAY\w*SCRATCH_BYTES", code)
    for name, count in SYMBOLS.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
    m = re.search(r"\bint64_t\s+pvamd_ray_cast_backward_scratch_bytes\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 4 == len(_lib.SIGNATURES["pvamd_ray_cast_backward_scratch_bytes"][1])
    makefile = open(os.path.join(ROOT, "pytorch_volumetric_amd", "csrc", "Makefile")).read()
    assert "ray_cast_backward.hip" in makefile


def test_scratch_size_is_the_librarys_plan():
    """pvamd_ray_cast_backward_scratch_bytes: 12 float64 per (chunk, leaf, configuration), rounded to 256 bytes, then 6 float64 per
    (split, ray) when the plan of the header's item 4 splits the configurations; the same for either element type; 0 for shapes
    the entry points refuse or have nothing to do for.  The binding asks the library and computes nothing itself."""
    lib = _lib.load()
    chunk = _lib.RAY_BACKWARD_CHUNK
    for S, A, R in ((1, 1, 1), (3, 1, 257), (3, 3, 65), (8, 20, 19200), (3, 122, 4097), (2, 5, 2048 * chunk + 1)):
        nchunks = -(-R // chunk)
        want = min(A, -(-2048 // nchunks))
        aper = -(-A // want)
        nsplit = -(-A // aper)
        slab = -(-(nchunks * S * A * 12 * 8) // 256) * 256
        expect = slab + (nsplit * R * 6 * 8 if nsplit > 1 else 0)
        for f64 in (0, 1):
            assert lib.pvamd_ray_cast_backward_scratch_bytes(S, A, R, f64) == expect, (S, A, R)
            assert _lib.ray_cast_backward_scratch_bytes(S, A, R, bool(f64)) == expect
    assert lib.pvamd_ray_cast_backward_scratch_bytes(0, 1, 1, 0) == 0 and lib.pvamd_ray_cast_backward_scratch_bytes(1, 0, 1, 0) == 0
    source = inspect.getsource(_lib.ray_cast_backward_scratch_bytes)
    assert "load().pvamd_ray_cast_backward_scratch_bytes(" in source
    assert not any(op in source.split('"""')[2] for op in ("//", "*", "+"))
