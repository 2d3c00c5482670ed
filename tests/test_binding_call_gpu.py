"""GPU: _lib.call against a real entry point -- the bits of the usual path, NULL for None, and every refusal before a launch."""
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def ball():
    """A sphere cached on the smallest lattice a grid descriptor takes (two voxels per axis), five points of which the last two
    are out of range, and what cached(points) answers."""
    cached = pv.CachedSDF("ball", 1.0, [(-0.5, 0.5)] * 3, pv.SphereSDF(0.4), device="cuda", cache_path=None)
    assert tuple(cached._view.shape) == (2, 2, 2)
    points = torch.tensor([[0.1, 0.2, -0.3], [-0.4, 0.4, 0.4], [0.3, -0.2, 0.1], [2.0, 0.0, 0.0], [-1.0, -3.0, 0.5]], device="cuda")
    val, grad = cached(points)
    return cached, points, val.clone(), grad.clone()


def outputs(dtype=torch.float32):
    return (torch.full((5,), SENTINEL, dtype=dtype, device="cuda"), torch.full((5, 3), SENTINEL, dtype=dtype, device="cuda"),
            torch.full((5,), 9, dtype=torch.uint8, device="cuda"))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_call_gives_the_bits_of_the_usual_path(ball):
    cached, points, want_val, want_grad = ball
    val, grad, oob = outputs()
    _lib.call("pvamd_cached_query", cached._grid_desc(), points, 5, val, grad, oob)
    assert same_bits(val, want_val) and same_bits(grad, want_grad)
    assert oob.tolist() == [0, 0, 0, 1, 1]


def test_none_passes_null(ball):
    cached, points, want_val, want_grad = ball
    val, grad, oob = outputs()
    _lib.call("pvamd_cached_query", cached._grid_desc(), points, 5, val, grad, None)
    assert same_bits(val, want_val) and same_bits(grad, want_grad)
    val64, grad64, _ = outputs(torch.float64)
    _lib.call("pvamd_cached_query", cached._grid_desc(), points.double(), 5, val64, grad64, None, f64=True)
    want64 = cached(points.double())
    assert torch.equal(val64, want64[0]) and torch.equal(grad64, want64[1])


@pytest.mark.parametrize("case", ["float64 points to the float32 entry", "float32 points to the float64 entry",
                                  "a transposed view as points"])
def test_a_refused_tensor_names_its_parameter_and_nothing_is_launched(ball, case):
    cached, points, _, _ = ball
    f64 = case == "float32 points to the float64 entry"
    val, grad, oob = outputs(torch.float64 if f64 else torch.float32)
    if case == "float64 points to the float32 entry":
        given, expected = points.double(), "torch.float32"
    elif f64:
        given, expected = points, "torch.float64"
    else:
        given, expected = points.t(), "torch.float32"  # the (3, P) view of the same storage
        assert given.shape == (3, 5) and not given.is_contiguous()
    name = "pvamd_cached_query" + ("_f64" if f64 else "")
    with pytest.raises(_lib.PvamdError, match=f"{name}: `points` takes a contiguous GPU tensor of {expected} or None, given a "
                                              f"{'non-' if case.startswith('a transposed') else ''}contiguous {given.dtype}"):
        _lib.call("pvamd_cached_query", cached._grid_desc(), given, 5, val, grad, oob, f64=f64)
    torch.cuda.synchronize()
    assert bool((val == SENTINEL).all()) and bool((grad == SENTINEL).all()) and bool((oob == 9).all())


def test_an_int32_tensor_for_an_int64_pointer_is_refused(ball):
    cached, points, _, _ = ball
    comp = pv.ComposedSDF([cached], None)
    comp.set_transforms(torch.eye(4, device="cuda").unsqueeze(0), batch_dim=(1,), known_rigid=True)
    want = comp.min_over_points(points)
    dev = points.device
    grids, tfd = comp._leaf_grids(dev), comp._tf_device(dev)
    scratch = _lib.scratch_buffer(_lib.min_over_points_scratch_bytes(1, 1, 5, False), dev)

    def buffers(index_dtype):
        return (torch.full((1, 1), SENTINEL, device=dev), torch.full((1, 1, 3), SENTINEL, device=dev),
                torch.full((1, 1), -5, dtype=index_dtype, device=dev), torch.full((1, 1), -5, dtype=torch.int32, device=dev))

    def run(out):
        _lib.call("pvamd_composed_min_over_points", grids, 1, tfd, 1, points, 5, _lib.LEAF_MODES["nearest"], False, *out, scratch)

    val, grad, index, leaf = out = buffers(torch.int64)  # the same call with the declared dtype runs
    run(out)
    assert same_bits(val.reshape(1), want.values) and same_bits(grad.reshape(1, 3), want.gradients)
    assert index.reshape(1).tolist() == want.indices.tolist() and leaf.item() == 0
    val, grad, index, leaf = out = buffers(torch.int32)
    with pytest.raises(_lib.PvamdError, match="pvamd_composed_min_over_points: `out_index` takes a contiguous GPU tensor of "
                                              "torch.int64 or None, given a contiguous torch.int32"):
        run(out)
    torch.cuda.synchronize()
    assert val.item() == SENTINEL and bool((grad == SENTINEL).all()) and index.item() == -5 and leaf.item() == -5
