"""The launch bounds of csrc, stated once, and the streaming kernels that no other test file takes past them.

Two bounds split a launch in csrc.  stream_grid() (common.h) caps a streaming grid at kNumCU x kMaxBlocksPerCU = 2048 blocks, so with
256 lanes a lane takes a second item only above H.STREAM_GRID_ITEMS = 524,288 items; and a grid's y dimension holds at most
H.GRID_Y_MAX = kMaxGridRows (common.h) rows, so kernels that carry the configuration in y wrap (a += gridDim.y) under a grid of
grid_rows() rows, or their host code walks slabs with for_row_slabs().
The first test below ties the two names to the sources.  The audit: every launch that `stream_grid(`, `kMaxGridRows`, `grid_rows(`,
`for_row_slabs(`, `gridDim.y` or `kMaxBlocksPerCU` finds in csrc, what its bound counts, and the test whose shape crosses it
("here" = this file, ITEMS =
H.STREAM_GRID_ITEMS, all other tests under tests/).  "not tested" without a reason: reachable in a few seconds (the same items in
two halves are a reference that needs no launch past the bound), no case yet.

    kernel (file)                                            bound                        crossed by
    -------------------------------------------------------  ---------------------------  ------------------------------------------
    voxel_gather / voxel_owner / voxel_scatter (voxelgrid)   points > ITEMS               test_voxelgrid_gpu::test_contested_scatter_and_gather_past_the_streaming_cap
    fill_i32_kernel (voxelgrid)                              voxels > ITEMS               test_voxelgrid_gpu::test_scatter_into_a_grid_of_more_voxels_than_the_streaming_cap
    edt_y_kernel, edt_x_kernel (distance_transform)          voxels > ITEMS               test_distance_transform_gpu::test_bit_for_bit_past_the_launch_caps
    edt_z_kernel (distance_transform)                        z lines > ITEMS / 64         same, and ::test_a_graph_replay_past_the_launch_caps_gives_the_eager_bits
    pack_grid_kernel (cached)                                voxels > ITEMS               test_wrench_fullsize_gpu::test_the_pickled_cache_is_the_reference_layout_and_reloads_bit_exact
                                                                                          (3,048,948 voxels repacked from the pickle)
    cached_query_scalar (cached)                             points > ITEMS               unreachable: chosen only below kWaveTileMinPoints points
    cached_outside_kernel, voxel_index_kernel (cached)       points > ITEMS               here::test_outside_surface_and_index_keys_past_the_streaming_cap (float32 range)
    cached_outside_f64_kernel, voxel_index_f64_kernel        points > ITEMS               not tested
    cached_backward_kernel (backward)                        points > ITEMS               not tested
    reduce_tf_kernel (tf_reduce.h: backward,                 S A 16 > ITEMS               here::test_composed_stack_gradient_past_the_streaming_cap (<float, float>),
    ray_cast_backward)                                                                    here::test_ray_cast_stack_gradient_past_the_streaming_cap (<double, float>)
    reduce_splits_kernel (backward)                          P 3 > ITEMS                  test_autograd_edges_gpu::test_composed_uneven_splits_300k (composed),
                                                                                          test_hinge_over_points_gpu::test_per_leaf_dpoints_of_more_points_than_the_reduction_grids_have_lanes
    accumulate_kernel (backward)                             P 3 > ITEMS                  the same hinge test
    mop_backward_kernel, mop scatter (min_over_points)       A Z pairs > ITEMS            not tested: unreachable in a few seconds (more than 524,288 (configuration, leaf) pairs)
    sample_surface_kernel (sample)                           samples > ITEMS              here::test_sample_surface_past_the_streaming_cap
    transform_points_kernel, compose_merge_kernel (composed) points > ITEMS               here::test_transform_points_past_the_streaming_cap,
                                                                                          here::test_mesh_leaves_past_the_streaming_cap_match_the_oracle_and_two_halves
                                                             A in y: for_row_slabs        here::test_transform_points_takes_more_transforms_than_grid_rows,
                                                                                          here::test_compose_merge_takes_more_configurations_than_grid_rows,
                                                                                          here::test_generic_leaves_under_more_configurations_than_grid_rows
    chamfer_grid_kernel (chamfer_grid)                       points > ITEMS / B per row;  test_chamfer_gpu::test_chamfer_grid_past_the_slab_and_the_streaming_cap
                                                             B in y: for_row_slabs
    chamfer_mesh_kernel (mesh)                               B in y: for_row_slabs        test_chamfer_gpu::test_chamfer_mesh_takes_more_transforms_than_one_grid_dimension_holds
    mesh part kernels (mesh)                                 parts > GRID_Y_MAX           unreachable: a mesh of more than 16.7 M triangles
    reg_partial_kernel, normal_eq_finish_kernel (registration) B > GRID_Y_MAX; B 29 > ITEMS  test_registration_gpu::test_more_poses_than_one_grid_dimension_holds
    lp_transform_kernel (leaf_pair)                          A K > ITEMS                  not tested
    lp_backward_kernel (leaf_pair)                           A K > ITEMS                  not tested
    lph_pair_vjp_kernel (leaf_pair)                          A K > ITEMS                  not tested
    lp_accumulate_kernel (leaf_pair)                         S A > ITEMS                  not tested: more than 65,536 robot configurations through forward kinematics and back
    lp_partial / lph_partial kernels (leaf_pair)             a += gridDim.y, at most      test_self_collision_gpu::test_bit_equal_to_one_leaf_min_over_points[200-*] and
                                                             4096 / (K chunks) rows       test_leaf_pair_hinge_gpu::test_bit_equal_to_one_leaf_hinge[200-*]: 56 pairs, 25 or 74 rows for 200
    cached_ray_cast_backward_kernel (ray_cast_backward)      rays > 2048 kRayBwdBlock     test_ray_cast_backward_gpu::test_cached_with_more_rays_than_the_backward_grid_has_lanes
    ray_reduce_rows_kernel (ray_cast_backward)               R 6 > ITEMS                  not tested
    mop_partial_kernel (min_over_points)                     A > GRID_Y_MAX               test_min_over_points_gpu::test_more_configurations_than_grid_rows
    hop_partial_kernel (hinge_over_points)                   A > GRID_Y_MAX               test_hinge_over_points_gpu::test_more_configurations_than_grid_rows
    composed_ray_cast_kernel (ray_cast)                      A > GRID_Y_MAX               test_ray_cast_gpu::test_more_configurations_than_grid_rows
    composed_interp_kernel (lane_query)                      A > GRID_Y_MAX               test_interp_gpu::test_composed_forward_with_more_configurations_than_grid_rows
    composed query kernels, slabs of A (composed)            A > GRID_Y_MAX               test_composed_gpu::test_seventy_thousand_configurations_go_out_in_slabs,
                                                                                          ::test_bucketed_and_packed_paths_take_more_than_65535_configurations
    composed_query_scalar, composed_query_wave (composed)    A x point blocks > 65536     not tested
    composed_query_f64_kernel (lane_query)                   A x point blocks > 65536     not tested
    composed_query_fused, grouped kernels (composed)         A x 4096-point chunks        not tested: more than 268 M (configuration, point) pairs, 4 GB of output
                                                             > 65536
    pvamd_composed_query_packed (composed)                   tile blocks > GRID_Y_MAX     refused (E_SHAPE): more than 67 M points in one call
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import oracle
from pytorch_volumetric_amd import _lib
from tests import helpers as H
from tests.test_min_over_points_gpu import same_bits

CSRC = os.path.join(os.path.dirname(os.path.abspath(pv.__file__)), "csrc")
PAST_CAP = H.PAST_CAP


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------- the bounds themselves (no GPU)
def test_the_bounds_the_tests_are_sized_by_are_the_sources_own():
    """A retuned cap must fail here, not silently leave the cases sized by H.STREAM_GRID_ITEMS and H.GRID_Y_MAX below the cap."""
    common = source("common.h")
    cus = int(re.search(r"constexpr\s+int\s+kNumCU\s*=\s*(\d+)\s*;", common).group(1))
    per_cu = int(re.search(r"constexpr\s+int\s+kMaxBlocksPerCU\s*=\s*(\d+)\s*;", common).group(1))
    assert re.search(r"const int64_t cap = \(int64_t\)kNumCU \* kMaxBlocksPerCU;\s*\n\s*return \(unsigned\)\(need < cap", common)
    assert cus * per_cu * 256 == H.STREAM_GRID_ITEMS  # every stream_grid(n, 256) launch: one item per lane up to here
    assert H.GRID_Y_MAX == 65535
    assert int(re.search(r"constexpr\s+int\s+kMaxGridRows\s*=\s*(\d+)\s*;", common).group(1)) == H.GRID_Y_MAX
    # the launches that clamp gridDim.y or walk slabs take the limit from common.h, in one of its three spellings; none has its own
    # (ray_cast.hip: the one place left is the width of the step counter, `max_steps > ...`, not a grid bound)
    for name in ("min_over_points.hip", "hinge_over_points.hip", "ray_cast.hip", "lane_query.hip", "registration.hip",
                 "chamfer_grid.hip", "mesh.hip", "composed.hip", "leaf_pair.hip"):
        text = source(name)
        assert re.search(r"kMaxGridRows|grid_rows\(|for_row_slabs\(", text), name
        assert str(H.GRID_Y_MAX) not in re.sub(r"max_steps > \d+", "", text), name
    # the distance transform's z pass: kEdtWaves lines per block of the same capped grid
    edt = source("distance_transform.hip")
    waves = int(re.search(r"constexpr\s+int\s+kEdtWaves\s*=\s*(\d+)\s*;", edt).group(1))
    assert cus * per_cu * waves == H.STREAM_GRID_ITEMS // 64  # lines one turn of the z pass covers
    # the streaming kernels with another block size
    assert re.search(r"stream_grid\(R,\s*kRayBwdBlock\)", source("ray_cast_backward.hip")) and _lib.RAY_BACKWARD_CHUNK == 256


# ---------------------------------------------------------------- GPU: the remaining streaming kernels past the cap
def analytic_cache(f64_range, resolution=0.01):
    return pv.CachedSDF("ellipsoid", resolution, H.padded_range(H.DRILL_BB, 0.05, as_numpy=f64_range), H.drill_like_gt(), device="cuda",
                        cache_path=None)


def spread_points(n, seed, margin=0.05):
    """In the caches' range and up to `margin` outside it."""
    r = H.padded_range(H.DRILL_BB, 0.05)
    return H.uniform_points(n, r[:, 0] - margin, r[:, 1] + margin, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2])
def test_transform_points_past_the_streaming_cap(A):
    lib = _lib.load()
    P = PAST_CAP
    tf = H.random_rigid(A, seed=40 + A, trans=0.2)
    pts = H.uniform_points(P, [-0.5] * 3, [0.5] * 3, seed=41)
    x = torch.full((A, P, 3), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.pvamd_transform_points(_lib.ptr(tf.cuda().contiguous()), A, _lib.ptr(pts.cuda().contiguous()), P, _lib.ptr(x),
                                          _lib.stream_ptr()), "pvamd_transform_points")
    want = oracle.transform_points(tf.numpy(), pts.numpy())
    assert same_bits(x.cpu().numpy(), want)


# ---------------------------------------------------------------- GPU: the glue entry points past the grid's rows
MANY = H.GRID_Y_MAX + 66  # the glue kernels take the configuration from blockIdx.y: rows 65535.. are the entry point's second slab
EDGE_ROWS = (0, 1, H.GRID_Y_MAX - 1, H.GRID_Y_MAX, H.GRID_Y_MAX + 1, MANY - 1)
MERGE_SEED = 48  # test_compose_merge_*: both leaves win among the rows of the second slab (asserted there, on the oracle's result)


@pytest.mark.gpu
def test_transform_points_takes_more_transforms_than_grid_rows():
    """pvamd_transform_points at the C ABI with more transforms than a grid has rows (refused with E_SHAPE before the entry point
    walked the slabs itself), into an output pre-filled with a value it never writes."""
    A, P = MANY, 5
    tf = H.random_rigid(A, seed=46, trans=0.2)
    pts = H.uniform_points(P, [-0.5] * 3, [0.5] * 3, seed=47)
    x = torch.full((A, P, 3), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().pvamd_transform_points(_lib.ptr(tf.cuda().contiguous()), A, _lib.ptr(pts.cuda().contiguous()), P, _lib.ptr(x),
                                                  _lib.stream_ptr()), "pvamd_transform_points")
    got, want = x.cpu().numpy(), oracle.transform_points(tf.numpy(), pts.numpy())
    for a in EDGE_ROWS:  # either side of the slab boundary, by name
        assert same_bits(got[a], want[a]), a
    assert same_bits(got, want)


@pytest.mark.gpu
def test_compose_merge_takes_more_configurations_than_grid_rows():
    """pvamd_compose_merge at the C ABI: two leaves folded (first = 1, then 0) with best_leaf, random values with NaNs in either
    leaf and in both, more configurations than a grid has rows."""
    lib = _lib.load()
    A, P = MANY, 5
    tf = H.random_rigid(2 * A, seed=MERGE_SEED, trans=0.2).reshape(2, A, 4, 4)
    rng = np.random.default_rng(MERGE_SEED)
    leaf_v = rng.standard_normal((2, A, P)).astype(np.float32)
    leaf_g = rng.standard_normal((2, A, P, 3)).astype(np.float32)
    leaf_v[0, [3, H.GRID_Y_MAX, MANY - 2], [0, 1, 2]] = np.nan  # NaN against a number, either way round, and against NaN
    leaf_v[1, [4, H.GRID_Y_MAX + 1, MANY - 2], [0, 1, 2]] = np.nan
    want_v, want_g = np.full((A, P), -7.0, np.float32), np.full((A, P, 3), -7.0, np.float32)
    want_leaf = np.full((A, P), -7, np.int32)
    best_v = torch.full((A, P), -7.0, dtype=torch.float32, device="cuda")
    best_g = torch.full((A, P, 3), -7.0, dtype=torch.float32, device="cuda")
    best_leaf = torch.full((A, P), -7, dtype=torch.int32, device="cuda")
    for s in range(2):
        oracle.compose_merge(tf[s].numpy(), leaf_v[s], leaf_g[s], s, want_v, want_g, want_leaf)
        tf_s, v, g = tf[s].cuda().contiguous(), torch.from_numpy(leaf_v[s]).cuda(), torch.from_numpy(leaf_g[s]).cuda()
        _lib.check(lib.pvamd_compose_merge(_lib.ptr(tf_s), A, P, _lib.ptr(v), _lib.ptr(g), s, 1 if s == 0 else 0, _lib.ptr(best_v),
                                           _lib.ptr(best_g), _lib.ptr(best_leaf), _lib.stream_ptr()), "pvamd_compose_merge")
    assert set(np.unique(want_leaf[H.GRID_Y_MAX:])) == {0, 1}  # both leaves win among the rows of the second slab
    assert np.isnan(want_v[MANY - 2, 2]) and want_leaf[H.GRID_Y_MAX, 1] == 0 and want_leaf[H.GRID_Y_MAX + 1, 1] == 1
    assert np.array_equal(best_leaf.cpu().numpy(), want_leaf)
    assert same_bits(best_v.cpu().numpy(), want_v) and same_bits(best_g.cpu().numpy(), want_g)


@pytest.mark.gpu
def test_generic_leaves_under_more_configurations_than_grid_rows():
    """ComposedSDF over leaves that are no cached grids (pvamd_transform_points -> the leaf -> pvamd_compose_merge) under more
    configurations than a grid has rows, against the same stack queried as two batches that each stay below that."""
    A, P = MANY, 3
    tfm = H.random_rigid(2 * A, seed=49, trans=0.2).reshape(2, A, 4, 4)
    pts = H.uniform_points(P, [-0.3] * 3, [0.3] * 3, seed=50).cuda()

    def query(rows):
        comp = pv.ComposedSDF([pv.SphereSDF(0.1), pv.SphereSDF(0.2)], None)
        comp.set_transforms(tfm[:, rows].reshape(-1, 4, 4).cuda(), batch_dim=(tfm[:, rows].shape[1],))
        return comp(pts)

    val, grad = query(slice(None))
    assert val.shape == (A, P) and grad.shape == (A, P, 3)
    half = A // 2
    assert half < H.GRID_Y_MAX and A - half < H.GRID_Y_MAX
    (va, ga), (vb, gb) = query(slice(0, half)), query(slice(half, None))
    assert same_bits(val.cpu().numpy(), torch.cat((va, vb)).cpu().numpy())
    assert same_bits(grad.cpu().numpy(), torch.cat((ga, gb)).cpu().numpy())
    assert len(np.unique(val[H.GRID_Y_MAX:].cpu().numpy())) > 100  # the configurations of the second slab do differ


@pytest.mark.gpu
def test_mesh_leaves_past_the_streaming_cap_match_the_oracle_and_two_halves():
    """ComposedSDF over MeshSDF leaves: pvamd_transform_points -> the mesh kernel -> pvamd_compose_merge, one configuration, more
    points than the capped grids of the two glue kernels have lanes.  Against the composition stated with the oracle's pieces
    (tests/test_composed_gpu.py does this at 4000 points), and against the same points queried in two halves."""
    objs = [pv.MeshObjectFactory(H.mesh_path("box_template.obj"), scale=0.03), pv.MeshObjectFactory(H.mesh_path("box_template.obj"), scale=0.02)]
    S, P = 2, PAST_CAP
    tfm = H.random_rigid(S, seed=43, trans=0.05)
    comp = pv.ComposedSDF([pv.MeshSDF(o) for o in objs], None)
    comp.set_transforms(pv.Transform3d(matrix=tfm), batch_dim=(1,))
    pts = H.uniform_points(P, [-0.1] * 3, [0.1] * 3, seed=44)
    dev = pts.cuda()
    val, grad = comp(dev)
    assert val.shape == (1, P) and grad.shape == (1, P, 3)
    half = P // 2
    assert half < H.STREAM_GRID_ITEMS
    (va, ga), (vb, gb) = comp(dev[:half]), comp(dev[half:])
    assert same_bits(val.cpu().numpy(), torch.cat((va, vb), dim=1).cpu().numpy())
    assert same_bits(grad.cpu().numpy(), torch.cat((ga, gb), dim=1).cpu().numpy())
    best_v, best_g = np.full((1, P), -7.0, np.float32), np.full((1, P, 3), -7.0, np.float32)
    best_leaf = np.full((1, P), -7, np.int32)
    for s, obj in enumerate(objs):
        tf_s = tfm.reshape(S, 1, 4, 4)[s].numpy()
        x = oracle.transform_points(tf_s, pts.numpy())
        _, d, g, _, _ = oracle.mesh_query(H.oracle_mesh_from_factory(obj), x.reshape(-1, 3), seed=obj.jitter_seed)
        oracle.compose_merge(tf_s, d.reshape(1, P), g.reshape(1, P, 3), s, best_v, best_g, best_leaf)
    assert same_bits(val.cpu().numpy(), best_v) and same_bits(grad.cpu().numpy(), best_g)
    assert len(np.unique(best_leaf[0, H.STREAM_GRID_ITEMS:])) == 2  # both leaves win among the points of the second turn


# ---------------------------------------------------------------- GPU: the stack gradient's finish kernel past the cap
TF_A = 16_400  # two leaves: S A 16 = 524,800 entries of dtf, 512 past the cap; each half of the configurations stays below it
TF_POINTS = 64


@pytest.fixture(scope="module")
def two_leaves_and_a_stack():
    """Two small analytic caches under TF_A rigid configurations, leaf-major (2, TF_A, 4, 4)."""
    S = 2
    assert S * TF_A * 16 > H.STREAM_GRID_ITEMS >= S * (TF_A // 2) * 16 and TF_A % 2 == 0
    return [analytic_cache(False, 0.02) for _ in range(S)], H.random_rigid(S * TF_A, seed=51, trans=0.05).reshape(S, TF_A, 4, 4)


def stack_gradient_whole_and_in_halves(stack, gradient_of):
    """gradient_of(rows) -> the (S, len(rows), 4, 4) gradient w.r.t. the stack of the configurations `rows` alone.  A row
    dtf[s, a] is a sum over the points or rays of configuration a only, so the halves are a reference for the whole."""
    S, A, half = stack.shape[0], stack.shape[1], stack.shape[1] // 2
    whole = gradient_of(slice(None))
    halves = torch.cat((gradient_of(slice(0, half)), gradient_of(slice(half, None))), dim=1)
    assert whole.shape == halves.shape == (S, A, 4, 4)
    second_turn = whole.reshape(-1)[H.STREAM_GRID_ITEMS:]  # the entries a lane of reduce_tf_kernel takes second
    assert second_turn.numel() == S * A * 16 - H.STREAM_GRID_ITEMS and bool((second_turn != 0).any())
    share = float((whole[:, :, :3] != 0).any(dim=3).any(dim=2).float().mean())  # (leaf, configuration) rows that receive a term
    print(f"rows of dtf with a term: {share:.3f}, non-zero entries of the second turn: {int((second_turn != 0).sum())}")
    assert bool((whole[:, :, 3] == 0).all()) and share > 0.25
    assert same_bits(whole.cpu().numpy(), halves.cpu().numpy())


@pytest.mark.gpu
def test_composed_stack_gradient_past_the_streaming_cap(two_leaves_and_a_stack):
    """reduce_tf_kernel<float, float> (csrc/tf_reduce.h) behind the composed backward: a value-only upstream, float32."""
    leaves, stack = two_leaves_and_a_stack
    pts = spread_points(TF_POINTS, seed=52, margin=0.1).cuda()
    up = torch.randn((TF_A, TF_POINTS), generator=torch.Generator().manual_seed(53)).cuda()

    def gradient_of(rows):
        m = stack[:, rows].reshape(-1, 4, 4).cuda().requires_grad_()
        comp = pv.ComposedSDF(leaves, None)
        comp.set_transforms(m, batch_dim=(m.shape[0] // 2,))
        val, _ = comp(pts)
        return torch.autograd.grad((val * up[rows]).sum(), m)[0].reshape(2, -1, 4, 4)

    stack_gradient_whole_and_in_halves(stack, gradient_of)


@pytest.mark.gpu
def test_ray_cast_stack_gradient_past_the_streaming_cap(two_leaves_and_a_stack):
    """reduce_tf_kernel<double, float> behind the ray-cast backward: 64 rays from a sphere around the leaves towards them."""
    leaves, stack = two_leaves_and_a_stack
    rng = np.random.default_rng(54)
    o = rng.normal(size=(TF_POINTS, 3))
    o = 0.8 * o / np.linalg.norm(o, axis=-1, keepdims=True)
    d = rng.uniform(-0.08, 0.08, size=(TF_POINTS, 3)) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o, d = torch.from_numpy(o).float().cuda(), torch.from_numpy(d).float().cuda()
    up = (torch.rand((TF_A, TF_POINTS), generator=torch.Generator().manual_seed(55)) + 0.5).cuda()

    def gradient_of(rows):
        m = stack[:, rows].reshape(-1, 4, 4).cuda().requires_grad_()
        comp = pv.ComposedSDF(leaves, None)
        comp.set_transforms(m, batch_dim=(m.shape[0] // 2,))
        res = comp.ray_cast(o, d, differentiable=True, t_max=2.0, max_steps=32)
        return torch.autograd.grad((res.t * up[rows]).sum(), m)[0].reshape(2, -1, 4, 4)

    stack_gradient_whole_and_in_halves(stack, gradient_of)


@pytest.mark.gpu
def test_sample_surface_past_the_streaming_cap():
    obj = pv.MeshObjectFactory(H.mesh_path("box_template.obj"))
    n = PAST_CAP
    obj.sample_surface(8, seed=1)  # builds the triangle and area tables
    tri, cdf = obj._tri_dev, obj._area_cdf_dev
    pts = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda")
    face = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    keys = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().pvamd_sample_surface(_lib.ptr(tri), _lib.ptr(cdf), int(tri.shape[0]), n, ctypes.c_uint64(123), _lib.ptr(pts),
                                                _lib.ptr(face), _lib.ptr(keys), _lib.stream_ptr()), "pvamd_sample_surface")
    opts, oface, okeys = oracle.sample_surface(tri.cpu().numpy(), cdf.cpu().numpy(), n, 123)
    assert np.array_equal(pts.cpu().numpy(), opts) and np.array_equal(face.cpu().numpy(), oface)
    assert np.array_equal(keys.cpu().numpy(), okeys) and (okeys >= 0).all()
    p2, f2, k2 = obj.sample_surface(n, seed=123)  # and through the factory
    assert torch.equal(p2, pts) and torch.equal(f2, face) and torch.equal(k2, keys)


@pytest.mark.gpu
def test_outside_surface_and_index_keys_past_the_streaming_cap():
    """pvamd_cached_outside and pvamd_voxel_index (float32 range, float32 points) into outputs pre-filled with values they never
    write, against the oracle."""
    lib = _lib.load()
    cached = analytic_cache(False)
    og = H.oracle_grid_from_cached(cached)
    P = PAST_CAP
    pts = spread_points(P, seed=45)
    host = pts.numpy()
    level = 0.01
    want_out = oracle.cached_outside(og, host, level)
    want_key, want_flat, want_valid = oracle.voxel_index(og, host)
    assert 0.2 < want_valid.mean() < 0.8 and 0.05 < want_out[want_valid].mean() < 0.95
    assert want_valid[H.STREAM_GRID_ITEMS:].any()
    dev = pts.cuda().contiguous()
    desc = cached._grid_desc()
    out = torch.full((P,), 7, dtype=torch.uint8, device="cuda")
    _lib.check(lib.pvamd_cached_outside(ctypes.byref(desc), _lib.ptr(dev), P, level, _lib.ptr(out), _lib.stream_ptr()),
               "pvamd_cached_outside")
    assert np.array_equal(out.cpu().numpy(), want_out.astype(np.uint8))
    key = torch.full((P, 3), -7, dtype=torch.int64, device="cuda")
    flat = torch.full((P,), -7, dtype=torch.int64, device="cuda")
    valid = torch.full((P,), 7, dtype=torch.uint8, device="cuda")
    _lib.check(lib.pvamd_voxel_index(ctypes.byref(desc), _lib.ptr(dev), P, _lib.ptr(key), _lib.ptr(flat), _lib.ptr(valid),
                                     _lib.stream_ptr()), "pvamd_voxel_index")
    assert np.array_equal(valid.cpu().numpy(), want_valid.astype(np.uint8))
    assert np.array_equal(key.cpu().numpy(), want_key)
    assert np.array_equal(flat.cpu().numpy()[want_valid], want_flat[want_valid])  # of a point without a voxel: unspecified
