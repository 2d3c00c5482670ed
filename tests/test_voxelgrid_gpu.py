"""-m gpu: VoxelGrid / ExpandingVoxelGrid / voxel_down_sample on the HIP gather / scatter kernels (SURVEY 8(f) rank 4,
reference voxel.py:42-171) vs the oracle's restatement and vs the generic torch path of the same container."""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import oracle
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd.voxel_containers import ValueRangeView
from tests import helpers as H

pytestmark = pytest.mark.gpu


def oracle_grid_of(vg):
    """the oracle's view of a VoxelGrid's (or a bare ValueRangeView's) index arithmetic, under the index rule the view was
    built with (storage handled in numpy by the caller)"""
    view = getattr(vg, "voxels", vg)
    shape = view.shape
    rmin = np.array([b[0] for b in view._ranges])
    rmax = np.array([b[1] for b in view._ranges])
    f64 = view._min.dtype == torch.float64
    dt = np.float64 if f64 else np.float32
    dummy = np.zeros(shape, np.float32)
    return oracle.Grid(dummy, np.zeros((dummy.size, 3), np.float32), rmin.astype(dt), rmax.astype(dt), np.zeros((3, 2)),
                       index_f64=f64, rule=view._rule)


@pytest.mark.parametrize("f64_range", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bool])
def test_scatter_then_gather_matches_oracle(f64_range, dtype):
    rng = np.random.default_rng(3)
    lo, hi = np.array([-0.31, 0.07, 1.2]), np.array([0.45, 0.62, 1.9])
    ranges = np.stack((lo, hi), axis=1) if f64_range else [(float(a), float(b)) for a, b in zip(lo, hi)]
    vg = pv.VoxelGrid(0.013, ranges, dtype=dtype, device="cuda")
    assert vg.voxels._device_path(torch.zeros(1, 3, device="cuda"))
    og = oracle_grid_of(vg)
    P = 200_000
    pts = (lo - 0.1 + rng.random((P, 3)) * (hi - lo + 0.2)).astype(np.float32)  # ~40 % out of range, many duplicates
    pts[:500] = pts[500:1000]                                                    # exact duplicates, different values
    store = np.zeros(vg.voxels.shape, np.float32 if dtype == torch.float32 else np.bool_)
    if dtype == torch.float32:
        vals = rng.normal(size=P).astype(np.float32)
        vg[torch.from_numpy(pts).cuda()] = torch.from_numpy(vals).cuda()
        oracle.voxel_scatter(og, store, pts, vals)
    else:
        vg[torch.from_numpy(pts).cuda()] = 1
        oracle.voxel_scatter(og, store, pts, True)
    assert np.array_equal(vg.get_voxel_values().cpu().numpy(), store), "scatter: last writer in input order must win"
    q = (lo - 0.2 + rng.random((50_000, 3)) * (hi - lo + 0.4)).astype(np.float32)
    got = vg[torch.from_numpy(q).cuda()].cpu().numpy()
    assert np.array_equal(got, oracle.voxel_gather(og, store, q, 0))
    # batch dimensions carry through
    assert vg[torch.from_numpy(q).cuda().reshape(50, 1000, 3)].shape == (50, 1000)


def test_device_path_equals_the_generic_torch_path():
    """same container, storage on the CPU -> generic torch path; must agree with the HIP path bit for bit (one writer
    per voxel: torch's own index assignment does not define which of several writers wins)"""
    rng = np.random.default_rng(5)
    ranges = [(-1.0, 1.0), (-0.5, 0.5), (0.0, 0.7)]
    a, b = pv.VoxelGrid(0.05, ranges, device="cuda"), pv.VoxelGrid(0.05, ranges, device="cpu")
    centres = b.get_voxel_center_points()
    pick = torch.from_numpy(rng.permutation(len(centres))[:3000])
    pts = centres[pick] + torch.from_numpy(rng.uniform(-0.02, 0.02, (3000, 3)).astype(np.float32))
    pts = torch.cat((pts, torch.from_numpy(rng.uniform(1.3, 2.0, (500, 3)).astype(np.float32))))  # out of range: ignored
    vals = torch.from_numpy(rng.normal(size=3500).astype(np.float32))
    a[pts.cuda()] = vals.cuda()
    b[pts] = vals
    assert torch.equal(a.get_voxel_values().cpu(), b.get_voxel_values())
    assert torch.equal(a[pts.cuda()].cpu(), b[pts])
    pa, va = a.get_known_pos_and_values()
    pb, vb = b.get_known_pos_and_values()
    assert torch.equal(pa.cpu(), pb) and torch.equal(va.cpu(), vb)


def test_expanding_grid_and_down_sample_on_device():
    rng = np.random.default_rng(1)
    g = pv.ExpandingVoxelGrid(0.1, [(0.0, 1.0)] * 3, device="cuda")
    inside = torch.tensor([[0.5, 0.5, 0.5], [0.21, 0.88, 0.07]], device="cuda")
    g[inside] = torch.tensor([2.0, 3.0], device="cuda")
    far = torch.tensor([[1.73, -0.42, 0.5]], device="cuda")
    g[far] = torch.tensor([5.0], device="cuda")          # grows the range, keeps what was known
    assert g[inside].tolist() == [2.0, 3.0] and g[far].tolist() == [5.0]
    assert g.range_per_dim[0][1] >= 1.73 and g.range_per_dim[1][0] <= -0.42
    # down-sampling: one centre per occupied cell, every point within half a cell diagonal of a centre (test_voxel_sdf.py:29)
    cloud = torch.from_numpy(rng.normal(size=(200_000, 3)).astype(np.float32) * np.array([0.3, 0.2, 0.1], np.float32)).cuda()
    res = 0.02
    centres = pv.voxel_down_sample(cloud, res)
    on_cpu = pv.voxel_down_sample(cloud.cpu(), res)
    assert torch.equal(centres.cpu(), on_cpu)
    assert len(centres) < len(cloud)
    d = torch.cdist(cloud[:2000], centres).min(dim=1).values
    assert d.max().item() < res * np.sqrt(3) / 2 * 1.01


def test_cabi_rejects_missing_scratch_and_bad_shapes():
    lib = _lib.load()
    vg = pv.VoxelGrid(0.1, [(0.0, 1.0)] * 3, device="cuda")
    desc = vg.voxels._grid_desc()
    pts = torch.zeros(4, 3, device="cuda")
    vals = torch.zeros(4, device="cuda")
    store = vg.get_voxel_values()
    rc = lib.pvamd_voxel_scatter_f32(ctypes.byref(desc), _lib.ptr(store), _lib.ptr(pts), _lib.ptr(vals), 0.0, 4, None,
                                     _lib.stream_ptr())
    assert rc == -1  # per-point values need the owner scratch
    assert lib.pvamd_voxel_gather_f32(ctypes.byref(desc), _lib.ptr(store), _lib.ptr(pts), -1, 0.0, _lib.ptr(vals),
                                      _lib.stream_ptr()) == -2
    assert lib.pvamd_voxel_gather_f32(ctypes.byref(desc), _lib.ptr(store), _lib.ptr(pts), 0, 0.0, None, _lib.stream_ptr()) == 0


# ---------------------------------------------------------------- past the streaming cap, the index edges, the argument forms
# (the audit of tests/test_launch_bounds.py: which launch bound each of these crosses)
PAST_CAP = H.PAST_CAP
INDEX_RULES = [0, pv.RULE_VALID_ON_INDEX, pv.RULE_ROUND_HALF_AWAY, pv.RULE_ROUND_FLOOR_HALF,
               pv.RULE_VALID_ON_INDEX | pv.RULE_ROUND_HALF_AWAY, pv.RULE_VALID_ON_INDEX | pv.RULE_ROUND_FLOOR_HALF,
               pv.RULE_RES_F64, pv.RULE_VALID_ON_INDEX | pv.RULE_RES_F64]  # the list tests/test_index_rules.py iterates


def ranged(lo, hi, f64_range):
    """value ranges whose element type selects float64 or float32 index arithmetic"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.stack((lo, hi), axis=1) if f64_range else [(float(a), float(b)) for a, b in zip(lo, hi)]


def gather_into_sentinel(vg, pts, invalid):
    """pvamd_voxel_gather_* into an output pre-filled with a value no voxel holds: an unwritten element shows"""
    view = vg.voxels
    as_bytes = view.dtype == torch.bool
    store = view.raw_data.view(torch.uint8) if as_bytes else view.raw_data
    out = torch.full((len(pts),), 0xAB if as_bytes else -777.0, dtype=store.dtype, device="cuda")
    fn = _lib.load().pvamd_voxel_gather_u8 if as_bytes else _lib.load().pvamd_voxel_gather_f32
    rc = fn(ctypes.byref(view._grid_desc()), _lib.ptr(store), _lib.ptr(pts), len(pts), int(invalid) if as_bytes else float(invalid),
            _lib.ptr(out), _lib.stream_ptr())
    assert rc == 0
    return out.cpu().numpy()


F64_RANGE = pytest.mark.parametrize("f64_range", [False, True], ids=["float32-range", "float64-range"])
SMALL_LO, SMALL_HI = np.array([-0.2, 0.1, 1.0]), np.array([0.2, 0.45, 1.3])  # 9 x 8 x 7 voxels of 0.05


@F64_RANGE
@pytest.mark.parametrize("kind", ["float-per-point", "bool-scalar", "bool-per-point"])
def test_contested_scatter_and_gather_past_the_streaming_cap(kind, f64_range):
    """More points than the capped grid has lanes, into 504 voxels.  The points of the second turn of the grid-stride loop
    come last in input order, so they are the last writers of nearly every voxel (per-point values), and the only writers
    of the upper z layers (scalar value): a loop that stops after its first turn leaves the storage wrong."""
    rng = np.random.default_rng(17)
    lo, hi = SMALL_LO, SMALL_HI
    dtype = torch.float32 if kind == "float-per-point" else torch.bool
    vg = pv.VoxelGrid(0.05, ranged(lo, hi, f64_range), dtype=dtype, device="cuda")
    assert vg.voxels.shape == (9, 8, 7) and (vg.voxels._min.dtype == torch.float64) == f64_range
    og = oracle_grid_of(vg)
    P, first = PAST_CAP, H.STREAM_GRID_ITEMS
    pts = (lo - 0.02 + rng.random((P, 3)) * (hi - lo + 0.04)).astype(np.float32)
    if kind == "bool-scalar":  # first turn: z below 1.14 only; second turn: z above it, and x below 0.1 (some voxels stay unset)
        pts[:first, 2] = (0.98 + rng.random(first) * 0.16).astype(np.float32)
        pts[first:, 2] = (1.16 + rng.random(P - first) * 0.16).astype(np.float32)
        pts[first:, 0] = (-0.22 + rng.random(P - first) * 0.3).astype(np.float32)
    _, flat, valid = oracle.voxel_index(og, pts)
    assert 0.2 < 1 - valid.mean() < 0.4  # about 30 % out of range
    store = np.zeros(vg.voxels.shape, np.float32 if dtype == torch.float32 else np.bool_)
    dpts = torch.from_numpy(pts).cuda()
    if kind == "bool-scalar":
        vg[dpts] = True
        oracle.voxel_scatter(og, store, pts, True)
        only_first = store.copy()
        only_first.reshape(-1)[flat[first:][valid[first:]]] = False
        assert store.sum() > only_first.sum() > 0 and not store.all()
    else:
        vals = rng.normal(size=P).astype(np.float32) if kind == "float-per-point" else rng.random(P) < 0.5
        vg[dpts] = torch.from_numpy(vals).cuda()
        oracle.voxel_scatter(og, store, pts, vals)
        assert len(np.unique(flat[first:][valid[first:]])) > 400  # the second turn owns most voxels
        assert store.all() if kind == "float-per-point" else (store.any() and not store.all())
    got = vg.get_voxel_values().cpu().numpy()
    assert np.array_equal(got, store), int((got != store).sum())
    want = oracle.voxel_gather(og, store, pts, 0)
    out = gather_into_sentinel(vg, dpts, 0)
    assert np.array_equal(out, want.astype(out.dtype)), int((out != want.astype(out.dtype)).sum())
    assert np.array_equal(vg[dpts].cpu().numpy(), want)


@F64_RANGE
def test_scatter_into_a_grid_of_more_voxels_than_the_streaming_cap(f64_range):
    """Per-point values clear one owner slot per voxel first (fill_i32_kernel): with more voxels than the capped grid has
    lanes that fill strides too.  The owner scratch starts as INT32_MAX here, which no point index exceeds: a slot the fill
    left alone would refuse its writer, and the points are the centres of the LAST voxels in storage order."""
    lo, hi = np.array([-0.2, 0.1, 1.0]), np.array([0.7, 0.9, 1.75])
    vg = pv.VoxelGrid(0.01, ranged(lo, hi, f64_range), device="cuda")
    nvox = vg.get_voxel_values().numel()
    assert vg.voxels.shape == (91, 81, 76) and nvox > H.STREAM_GRID_ITEMS
    og = oracle_grid_of(vg)
    rng = np.random.default_rng(23)
    P = 3000
    every = np.stack(np.unravel_index(np.arange(nvox), vg.voxels.shape), axis=1)
    interior = np.flatnonzero(((every > 0) & (every < np.array(vg.voxels.shape) - 1)).all(axis=1))  # the jitter stays in range
    tail = rng.permutation(interior[interior >= H.STREAM_GRID_ITEMS])[:P // 2]         # voxels of the fill's second turn
    anywhere = rng.permutation(interior[interior < H.STREAM_GRID_ITEMS])[:P - P // 2]
    idx = every[np.concatenate((tail, anywhere))]
    pts = (lo + idx * 0.01 + rng.uniform(-0.003, 0.003, (P, 3))).astype(np.float32)
    vals = rng.uniform(0.5, 1.5, P).astype(np.float32)
    store = np.zeros(vg.voxels.shape, np.float32)
    oracle.voxel_scatter(og, store, pts, vals)
    assert (store != 0).sum() == P and (store.reshape(-1)[H.STREAM_GRID_ITEMS:] != 0).sum() == P // 2
    dpts, dvals = torch.from_numpy(pts).cuda(), torch.from_numpy(vals).cuda()
    owner = torch.full((nvox,), 2 ** 31 - 1, dtype=torch.int32, device="cuda")
    raw = torch.zeros((nvox,), dtype=torch.float32, device="cuda")
    rc = _lib.load().pvamd_voxel_scatter_f32(ctypes.byref(vg.voxels._grid_desc()), _lib.ptr(raw), _lib.ptr(dpts), _lib.ptr(dvals), 0.0, P,
                                             _lib.ptr(owner), _lib.stream_ptr())
    assert rc == 0
    assert np.array_equal(raw.cpu().numpy(), store.reshape(-1))
    assert int((owner >= 0).sum()) == P
    vg[dpts] = dvals  # and through the container
    assert np.array_equal(vg.get_voxel_values().cpu().numpy(), store)
    assert np.array_equal(vg[dpts].cpu().numpy(), vals)


def edge_points(view):
    """The construction of test_half_voxel_boundaries_round_half_even (tests/test_cached_gpu.py) on a container's view: points on
    and next to the half-voxel planes, on the range ends and one float32 outside them; then rows with NaN, +inf and -inf in
    one coordinate or in all.  Returns (points float32, number of rows with a non-finite coordinate at the end)."""
    mn, mx, res = view._min.double().cpu().numpy(), view._max.double().cpu().numpy(), view._resolution.double().cpu().numpy()
    ks = np.arange(0, max(view.shape) + 1)
    base = [mn[None, :] + (ks[:, None] + off) * res[None, :] for off in (0.5, 0.5 - 1e-7, 0.5 + 1e-7, 0.0, 1.0)]
    pts = np.concatenate(base + [mn[None], mx[None], np.nextafter(mn.astype(np.float32), -10)[None].astype(np.float64),
                                 np.nextafter(mx.astype(np.float32), 10)[None].astype(np.float64)]).astype(np.float32)
    inside = ((mn + mx) / 2).astype(np.float32)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for d in range(3):
            row = inside.copy()
            row[d] = v
            bad.append(row)
        bad.append(np.full(3, v, np.float32))
    return np.concatenate((pts, np.array(bad, np.float32))), len(bad)


@F64_RANGE
@pytest.mark.parametrize("rule", INDEX_RULES)
def test_index_edges_and_non_finite_points_under_every_index_rule(rule, f64_range):
    from pytorch_volumetric_amd import voxel
    prev = voxel.INDEX_RULE
    try:
        voxel.INDEX_RULE = rule
        vg = pv.VoxelGrid(0.05, ranged(SMALL_LO, SMALL_HI, f64_range), device="cuda")
    finally:
        voxel.INDEX_RULE = prev
    assert vg.voxels._rule == rule and vg.voxels._grid_desc().rule == rule
    og = oracle_grid_of(vg)
    pts, nbad = edge_points(vg.voxels)
    P = len(pts)
    vals = np.arange(1, P + 1, dtype=np.float32)  # distinct and non-zero: the writer of every voxel is identified
    _, _, valid = oracle.voxel_index(og, pts)
    assert not valid[-nbad:].any() and valid[:-nbad].any() and not valid[:-nbad].all()
    store = np.full(vg.voxels.shape, -5.0, np.float32)
    vg.get_voxel_values().fill_(-5.0)
    oracle.voxel_scatter(og, store, pts, vals)
    dpts = torch.from_numpy(pts).cuda()
    vg[dpts] = torch.from_numpy(vals).cuda()
    got = vg.get_voxel_values().cpu().numpy()
    assert np.array_equal(got, store), int((got != store).sum())
    assert (got != -5.0).sum() == len(np.unique(oracle.voxel_index(og, pts)[1][valid]))  # the points without a voxel wrote nothing
    back = vg[dpts].cpu().numpy()
    assert np.array_equal(back, oracle.voxel_gather(og, store, pts, 0))
    assert (back[~valid] == 0).all() and (back[valid] > 0).all()  # invalid_value where there is no voxel
    # the generic torch path of the same container states the same rule
    assert np.array_equal(vg.voxels.get_valid_values(dpts).cpu().numpy(), valid)


@F64_RANGE
def test_a_non_zero_invalid_value_is_what_points_without_a_voxel_read(f64_range):
    rng = np.random.default_rng(29)
    ranges = ranged(SMALL_LO, SMALL_HI, f64_range)  # 9 x 8 x 7 voxels of 0.05: the storage shape below
    for dtype, invalid in ((torch.float32, -1.0), (torch.bool, 1)):
        host = rng.normal(size=(9, 8, 7)).astype(np.float32) if dtype == torch.float32 else rng.random((9, 8, 7)) < 0.5
        view = ValueRangeView(torch.from_numpy(host).cuda(), ranges, invalid_value=invalid)
        og = oracle_grid_of(view)
        edge, _ = edge_points(view)
        cloud = (SMALL_LO - 0.1 + rng.random((5000, 3)) * (SMALL_HI - SMALL_LO + 0.2)).astype(np.float32)
        pts = np.concatenate((cloud, edge))
        dpts = torch.from_numpy(pts).cuda()
        assert view._device_path(dpts)
        want = oracle.voxel_gather(og, host, pts, -1 if dtype == torch.float32 else True)
        got = view[dpts]
        assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)
        valid = oracle.voxel_index(og, pts)[2]
        assert (~valid).sum() > 1000 and (got.cpu().numpy()[~valid] == invalid).all()


def test_argument_forms_equal_the_contiguous_flat_call():
    rng = np.random.default_rng(31)
    ranges = ranged(SMALL_LO, SMALL_HI, False)
    P = 2000
    pts = torch.from_numpy((SMALL_LO - 0.02 + rng.random((P, 3)) * (SMALL_HI - SMALL_LO + 0.04)).astype(np.float32)).cuda()
    vals = torch.from_numpy(rng.normal(size=P)).cuda()  # float64
    assert vals.dtype == torch.float64

    def fresh():
        return pv.VoxelGrid(0.05, ranges, device="cuda")

    flat = fresh()
    flat[pts] = vals.float()
    base = flat.get_voxel_values().clone()
    assert (base != 0).any()
    # float64 values into the float32 grid: rounded once, like the cast above
    g = fresh()
    g[pts] = vals
    assert torch.equal(g.get_voxel_values(), base)
    # batch dimensions on points and values
    g = fresh()
    g[pts.reshape(50, 40, 3)] = vals.float().reshape(50, 40)
    assert torch.equal(g.get_voxel_values(), base)
    assert torch.equal(g[pts.reshape(50, 40, 3)], flat[pts].reshape(50, 40))
    # a non-contiguous view of the points, and of the values
    wide = torch.full((P, 6), 9.0, device="cuda")
    wide[:, :3] = pts
    spread = torch.zeros((P, 2), device="cuda")
    spread[:, 0] = vals.float()
    assert not wide[:, :3].is_contiguous() and not spread[:, 0].is_contiguous()
    g = fresh()
    g[wide[:, :3]] = spread[:, 0]
    assert torch.equal(g.get_voxel_values(), base)
    assert torch.equal(g[wide[:, :3]], flat[pts])
    # a 0-dim tensor is a scalar, on either device
    scalar = fresh()
    scalar[pts] = 2.5
    for value in (torch.tensor(2.5), torch.tensor(2.5, device="cuda"), torch.tensor(2.5, dtype=torch.float64)):
        g = fresh()
        g[pts] = value
        assert torch.equal(g.get_voxel_values(), scalar.get_voxel_values())
    assert 2.5 in scalar.get_voxel_values().unique().tolist() and set(scalar.get_voxel_values().unique().tolist()) <= {0.0, 2.5}


def test_mismatched_per_point_values_are_refused_before_any_launch():
    """The scatter kernel reads values[i] for every point i: a value tensor of another length must never reach it."""
    vg = pv.VoxelGrid(0.05, ranged(SMALL_LO, SMALL_HI, False), device="cuda")
    vg.get_voxel_values().fill_(4.0)
    P = 10
    pts = torch.from_numpy(np.linspace(SMALL_LO, SMALL_HI, P).astype(np.float32)).cuda()
    assert vg.voxels._device_path(pts)
    for n in (1, 3, P + 1):
        with pytest.raises(ValueError, match=rf"\b{n} values for {P} points"):
            vg[pts] = torch.ones(n, device="cuda")
        with pytest.raises(ValueError, match=rf"\b{n} values for {P} points"):
            vg[pts] = torch.ones(n)
    torch.cuda.synchronize()
    assert (vg.get_voxel_values() == 4.0).all()
    vg[pts] = torch.ones(P, device="cuda")
    assert (vg[pts] == 1.0).all()
    # a growing grid refuses before it grows: range and storage stay as they were
    ev = pv.ExpandingVoxelGrid(0.05, ranged(SMALL_LO, SMALL_HI, False), device="cuda")
    ev[pts] = torch.ones(P, device="cuda")
    before, kept = ev.range_per_dim.copy(), ev.get_voxel_values().clone()
    with pytest.raises(ValueError, match=rf"\b3 values for {P} points"):
        ev[pts + 1.0] = torch.ones(3, device="cuda")
    assert np.array_equal(ev.range_per_dim, before) and torch.equal(ev.get_voxel_values(), kept)


def test_cabi_refuses_more_points_than_an_owner_index_holds():
    lib = _lib.load()
    vg = pv.VoxelGrid(0.1, [(0.0, 1.0)] * 3, device="cuda")
    desc = vg.voxels._grid_desc()
    pts = torch.zeros(4, 3, device="cuda")
    vals = torch.zeros(4, device="cuda")
    owner = torch.zeros(vg.get_voxel_values().numel(), dtype=torch.int32, device="cuda")
    store = vg.get_voxel_values()
    for values in (vals, None):  # the check precedes any launch: the buffers are never read
        rc = lib.pvamd_voxel_scatter_f32(ctypes.byref(desc), _lib.ptr(store), _lib.ptr(pts), _lib.ptr(values), 1.0, 2 ** 31,
                                         _lib.ptr(owner), _lib.stream_ptr())
        assert rc == _lib.E_SHAPE
    torch.cuda.synchronize()
    assert (store == 0).all()


def test_growing_grid_equals_its_cpu_twin_after_every_write():
    """Three writes, each forcing growth on other faces; one writer per voxel (jitter below 0.4 of a cell around distinct
    centres), so torch's index assignment on the CPU is defined and must leave what the HIP scatter leaves."""
    res = 0.1
    rng = np.random.default_rng(37)
    dev, cpu = pv.ExpandingVoxelGrid(res, [(0.0, 1.0)] * 3, device="cuda"), pv.ExpandingVoxelGrid(res, [(0.0, 1.0)] * 3, device="cpu")
    boxes = [((-8, 18), (1, 10), (1, 10)),    # cells per axis: grows -x and +x
             ((1, 10), (-9, 18), (1, 10)),    # grows -y and +y
             ((1, 10), (1, 10), (-17, 9))]    # grows -z only
    written = set()
    for k, box in enumerate(boxes):
        cells = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in box], indexing="ij"), axis=-1).reshape(-1, 3)
        cells = cells[rng.permutation(len(cells))[:2000]]
        assert len(cells) == 2000
        pts = torch.from_numpy((cells * res + rng.uniform(-0.39 * res, 0.39 * res, cells.shape)).astype(np.float32))
        vals = torch.from_numpy(rng.uniform(0.5, 1.5, 2000).astype(np.float32))
        before = cpu.range_per_dim.copy()
        dev[pts.cuda()] = vals.cuda()
        cpu[pts] = vals
        grew = (cpu.range_per_dim[:, 0] < before[:, 0] - 0.5 * res, cpu.range_per_dim[:, 1] > before[:, 1] + 0.5 * res)
        assert [list(g) for g in grew] == [[[True, False, False], [True, False, False]], [[False, True, False], [False, True, False]],
                                           [[False, False, True], [False, False, False]]][k]
        assert np.array_equal(dev.range_per_dim, cpu.range_per_dim)
        written |= {tuple(c) for c in cells.tolist()}
        (pd, vd), (pc, vc) = dev.get_known_pos_and_values(), cpu.get_known_pos_and_values()
        assert len(vc) == len(written), (len(vc), len(written))
        assert torch.equal(pd.cpu(), pc) and torch.equal(vd.cpu(), vc)
        assert torch.equal(dev[pts.cuda()].cpu(), vals) and torch.equal(cpu[pts], vals)


