"""-m gpu: no entry point writes past the scratch the library's own size function reports.  Every byte-sized scratch of the
fused reductions and their backwards, of the mesh entry points and of the spatial sort is allocated by _lib.scratch_buffer; here it hands out the requested bytes in front of a
1 MiB tail of 0xA5 that belongs to the test, so an overrun shows up as a changed byte, never as a fault.  The shapes are the
smallest at which each layout changes (chunk boundaries, split configurations, the per-leaf hinge's extra term)."""
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu
TAIL = 1 << 20
FILL = 0xA5
S = 2
MARGIN = 0.2
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def leaves():
    """Two 16^3 BOUNDING_BOX caches of an analytic ellipsoid."""
    gt = H.AnalyticEllipsoidSDF([0.47, 0.47, 0.47], [0.3, 0.2, 0.35], [[0.1, 0.85]] * 3)
    out = [pv.CachedSDF(f"leaf{s}", 2.0 ** -4, [(0.0, 0.9375)] * 3, gt, device="cuda", cache_path=None) for s in range(S)]
    assert all(tuple(c._view.shape) == (16, 16, 16) for c in out)
    return out


@pytest.fixture
def guard(monkeypatch):
    handed = []

    def guarded(nbytes, dev):
        whole = torch.empty((nbytes + TAIL,), dtype=torch.uint8, device=dev)
        whole[nbytes:] = FILL
        handed.append((whole, nbytes))
        return whole[:nbytes]

    monkeypatch.setattr(_lib, "scratch_buffer", guarded)

    def check(at_least=1):
        torch.cuda.synchronize()
        assert len(handed) >= at_least, "no scratch buffer was requested"
        for whole, nbytes in handed:
            assert bool((whole[nbytes:] == FILL).all()), f"a kernel wrote past its {nbytes}-byte scratch"
        n = len(handed)
        handed.clear()
        return n

    return check


def composition(leaves, A, dtype, seed, grad=False):
    comp = pv.ComposedSDF(list(leaves), None)
    t = W.random_rigid(S * A, seed=seed, trans=0.3).to(dtype).cuda().requires_grad_(grad)
    comp.set_transforms(t, batch_dim=(A,))
    return comp, t


def points(P, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) * 1.6 - 0.3).to(dtype).cuda()


@DTYPES
@pytest.mark.parametrize("per_leaf", [False, True], ids=["composed", "per_leaf"])
@pytest.mark.parametrize("P", [4096, 4097])
def test_forwards_stay_inside_their_scratch(leaves, guard, dtype, per_leaf, P):
    comp, _ = composition(leaves, 3, dtype, seed=P)
    p = points(P, dtype, seed=1)
    comp.min_over_points(p, per_leaf=per_leaf)
    comp.hinge_over_points(p, MARGIN, per_leaf=per_leaf)
    assert guard(2) == 2


@DTYPES
@pytest.mark.parametrize("A,P", [(1, 1000), (3, 1025), (64, 33792)], ids=["no_split", "two_chunks", "two_per_split"])
def test_backwards_stay_inside_their_scratch(leaves, guard, dtype, A, P):
    comp, t = composition(leaves, A, dtype, seed=A, grad=True)
    p = points(P, dtype, seed=2).requires_grad_()
    val, grad = comp(p)
    torch.autograd.grad(val.sum() + grad.sum(), (p, t))
    guard()
    for per_leaf in (False, True):  # per_leaf with S = 2: the hinge's extra [P][3] term
        res = comp.min_over_points(p, per_leaf=per_leaf)
        torch.autograd.grad(res.values.sum() + res.gradients.sum(), (p, t))
        assert guard(2) == 2
        res = comp.hinge_over_points(p, MARGIN, per_leaf=per_leaf)
        torch.autograd.grad(res.values.sum(), (p, t))
        assert guard(2) == 2


@DTYPES
@pytest.mark.parametrize("largest", [1024, 1025, 4096, 4097])
def test_leaf_pairs_stay_inside_their_scratch(leaves, guard, dtype, largest):
    comp, t = composition(leaves, 3, dtype, seed=largest, grad=True)
    sets = [points(300, dtype, seed=3), points(largest, dtype, seed=4)]
    pairs = torch.tensor([[0, 1], [1, 0]])
    forward = 1 if largest > _lib.MOP_CHUNK else 0  # a set within one chunk: the single-pass forward takes no scratch
    res = comp.leaf_pair_distance(sets, pairs)
    torch.autograd.grad(res.values.sum() + res.gradients.sum(), t)
    assert guard() == forward + 1
    res = comp.leaf_pair_hinge(sets, pairs, MARGIN)
    torch.autograd.grad(res.values.sum(), t)
    assert guard() == forward + 1


@pytest.mark.parametrize("P", [16385, 65536, 786431, 786432, 806912, 1048576])
def test_spatial_sort_stays_inside_its_scratch(guard, P):
    """The first size that uses scratch (2^15 cells), 2^18 cells, the last counting-sort and the first radix size (192 tiles),
    197 tiles (one past a perfect square, where the number of supergroups rounds), 2^21 cells and a third radix pass."""
    pts = points(P, torch.float32, seed=P)
    order, inverse, spts = _lib.morton_order(pts, min_points=0, want_inverse=True, want_sorted=True)
    assert guard() == 1
    idx = torch.arange(P, device="cuda", dtype=torch.int32)
    assert torch.equal(torch.sort(order).values, idx)
    assert torch.equal(inverse[order.long()], idx)
    assert torch.equal(spts, pts[order.long()])


@pytest.fixture(scope="module")
def drill():
    obj = pv.MeshObjectFactory(H.mesh_path("ycb_power_drill.npz"))
    assert obj.num_faces == 15728
    return obj


@pytest.mark.parametrize("P,ordered", [(1, False), (16384, False), (16385, True), (8192 * 64, True)])
def test_mesh_query_stays_inside_its_scratch(drill, guard, P, ordered):
    """Without an order: the by-point part of the scratch up to its last entry (pvamd_mesh_query_unordered).  With one: the first
    size past it, and as many point groups as the scratch has slots, where the two-launch path writes the last slot.  Same bits
    as the single-launch scan that takes no scratch."""
    bb = drill.bounding_box(padding_ratio=0.3)
    pts = H.uniform_points(P, bb[:, 0], bb[:, 1], seed=P).float().cuda()
    order = _lib.morton_order(pts, min_points=0) if ordered else None
    outs = []
    try:
        for split in (True, False):
            drill.tile_split = split
            r = drill.object_frame_closest_point(pts, compute_normal=True, order=order)
            outs.append((r.closest, r.distance, r.gradient, r.normal, drill._last_face_ids))
            if split:
                assert guard() == 1 + int(ordered)  # the mesh scratch, and the sort's above
    finally:
        drill.tile_split = True
    guard(0)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_heavy_point_groups_stay_inside_the_mesh_scratch(guard):
    """The centre points of test_mesh_gpu's heavy-groups test: more heavy groups than the list has slots for."""
    from pytorch_volumetric_amd import mesh_io
    obj = pv.MeshObjectFactory(mesh=mesh_io.uv_sphere_mesh(0.1, 150, 120))
    g = torch.Generator().manual_seed(3)
    torch.rand(4096, 3, generator=g)
    many = ((torch.rand(9000 * 64, 3, generator=g) - 0.5) * 0.02).float().cuda().contiguous()
    obj.object_frame_closest_point(many[:140_000])
    assert guard() == 2  # the sort's and the mesh scratch
    pv.batch_chamfer_dist(torch.eye(4).unsqueeze(0), many, obj_factory=obj)
    assert guard() == 2


def test_cache_build_stays_inside_the_mesh_scratch(drill, guard):
    cached = pv.CachedSDF("drill", 0.02, drill.bounding_box(padding=0.013), pv.MeshSDF(drill), device="cuda", cache_path=None)
    assert cached._packed.shape[0] > 0
    assert guard() == 1
