"""CPU: the autograd layer's C-ABI (ABI 13: backward entry points, scratch-size query, argument checks that return before any
launch) and the routing flag ComposedSDF keeps from set_transforms (no GPU needed)."""
import ctypes

import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib, autograd

BACKWARD = ("pvamd_cached_query_backward", "pvamd_cached_query_backward_f64", "pvamd_composed_backward_scratch_bytes",
            "pvamd_composed_query_backward", "pvamd_composed_query_backward_f64", "pvamd_chamfer_grid_backward")


def test_abi_13_exports_the_backward_entry_points():
    assert _lib.ABI_VERSION == 13
    lib = _lib.load()
    assert lib.pvamd_abi_version() == 13
    for name in BACKWARD:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_scratch_size_covers_the_slabs():
    lib = _lib.load()
    S, A, P = 8, 200, 262144
    chunks = -(-P // 1024)
    f32 = lib.pvamd_composed_backward_scratch_bytes(S, A, P, 0)
    f64 = lib.pvamd_composed_backward_scratch_bytes(S, A, P, 1)
    assert f32 >= chunks * S * A * 12 * 4 and f64 >= 2 * chunks * S * A * 12 * 4 - 256
    assert lib.pvamd_composed_backward_scratch_bytes(0, A, P, 0) == 0
    # one configuration: no split of the configurations, so only the dtf slab
    assert lib.pvamd_composed_backward_scratch_bytes(1, 1, 1000, 0) == 256


def test_backward_argument_checks_before_any_launch():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    dummy = ctypes.c_void_p(16)
    # S outside 1..64, A < 1, P < 0: PVAMD_E_SHAPE
    for S, A, P in ((0, 1, 1), (65, 1, 1), (1, 0, 1), (1, 1, -1)):
        assert lib.pvamd_composed_query_backward(dummy, S, dummy, A, dummy, P, dummy, dummy, null, dummy, null, dummy, null) == -2
        assert lib.pvamd_composed_query_backward_f64(dummy, S, dummy, A, dummy, P, dummy, dummy, null, dummy, null, dummy, null) == -2
    # nothing wanted: nothing to do
    assert lib.pvamd_composed_query_backward(dummy, 2, dummy, 3, dummy, 10, dummy, dummy, null, null, null, null, null) == 0
    # upstream given but no leaf ids: PVAMD_E_NULL
    assert lib.pvamd_composed_query_backward(dummy, 2, dummy, 3, dummy, 10, null, dummy, null, dummy, null, dummy, null) == -1
    assert lib.pvamd_cached_query_backward(None, dummy, 10, dummy, null, dummy, null) == -1
    assert lib.pvamd_chamfer_grid_backward(None, dummy, 1, dummy, 10, 1.0, dummy, dummy, null, dummy, null) == -1
    # a LOOKUP_GT_SDF grid has no backward: PVAMD_E_MODE
    g = _lib.GridDesc()
    g.vox = 256
    g.shape[0] = g.shape[1] = g.shape[2] = 4
    g.oob_mode = _lib.OOB_LOOKUP_GT_SDF
    g.finalized = 1
    assert lib.pvamd_cached_query_backward(ctypes.byref(g), dummy, 10, dummy, null, dummy, null) == -4


def test_composed_routing_flag_is_set_by_set_transforms():
    comp = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
    assert comp._tf_grad is False
    m = torch.eye(4).repeat(2, 1, 1)
    comp.set_transforms(m)
    assert comp._tf_grad is False
    comp.set_transforms(m.clone().requires_grad_())
    assert comp._tf_grad is True
    comp.obj_frame_to_link_frame = pv.Transform3d(matrix=m)
    assert comp._tf_grad is False
    comp.set_transforms(None)
    assert comp._tf_grad is False


def test_backward_is_once_differentiable():
    """create_graph=True through any of the Functions raises instead of giving a wrong second derivative."""
    for fn in (autograd.CachedQuery, autograd.ComposedQuery, autograd.ChainConfigure, autograd.TransformStack,
               autograd.GridChamfer):
        assert fn.backward.__wrapped__ is not None  # functools.wraps of torch.autograd.function.once_differentiable


def test_transform_stack_backward_matches_autograd_on_cpu():
    """TransformStack's VJP (offset_inv @ rigid_inverse(link_world)) against torch autograd of the same statement."""
    S, A = 3, 4
    g = torch.Generator().manual_seed(0)
    from workloads import random_rigid
    off = random_rigid(S, seed=1)
    lw = random_rigid(S * A, seed=2).requires_grad_()
    contract = lambda x: off.repeat_interleave(A, 0) @ pv.transforms.rigid_inverse(x)
    up = torch.randn(S * A, 4, 4, generator=g)
    (got,) = torch.autograd.grad(autograd.TransformStack.apply(off, lw, contract), lw, up)
    (want,) = torch.autograd.grad(contract(lw), lw, up)
    assert torch.allclose(got, want, atol=1e-5)
    with pytest.raises(RuntimeError):
        (d,) = torch.autograd.grad(autograd.TransformStack.apply(off, lw, contract), lw, up, create_graph=True)
        d.sum().backward()
