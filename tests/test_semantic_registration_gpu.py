"""GPU: pv.semantic_normal_equations and refine_poses with semantics / targets / huber_delta (csrc/registration.hip
sem_partial_kernel) against include/pvamd.h "Semantic normal equations", its float64 restatement
tests/semantic_registration_ref.py and, where the options are switched off, the kernels of "Chamfer normal equations" bit for
bit.  The caches and helpers are those of test_registration_gpu.py: the drill at 0.01 m, both modes, both index arithmetics."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import registration as reg
from tests import registration_ref as R
from tests import semantic_registration_ref as S
from tests.test_min_over_points_gpu import deepest_voxel_centre
from tests.test_registration_gpu import (CHUNK, COUNTS, U, build_cache, cache_vn, caches, clouds, nearest, poses,  # noqa: F401
                                         transformed, tri)

pytestmark = pytest.mark.gpu

DELTA = 0.01
FIELDS = ("cost", "gradient", "hessian", "counts", "active", "outliers")


def run_sem(c, Wm, pts, kinds=None, targets=None, delta=math.inf):
    """pvamd_semantic_normal_eq through ctypes: (sums (B, 28) float64, counts (B, 5) int64) on the device."""
    B, N = Wm.shape[0], pts.shape[0]
    sums = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device="cuda")
    counts = torch.empty((B, _lib.SEM_COUNTS), dtype=torch.int64, device="cuda")
    scratch = _lib.scratch_buffer(_lib.semantic_normal_eq_scratch_bytes(B, N), "cuda")
    desc = c._grid_desc()
    _lib.check(_lib.load().pvamd_semantic_normal_eq(ctypes.byref(desc), _lib.LEAF_MODES[c.interpolation], _lib.ptr(Wm), B,
                                                    _lib.ptr(pts), N, _lib.ptr(kinds), _lib.ptr(targets), delta, _lib.ptr(sums),
                                                    _lib.ptr(counts), _lib.ptr(scratch), _lib.stream_ptr()),
               "pvamd_semantic_normal_eq")
    return sums, counts


def packed(ne, N, scale=1000.):
    """(B, 28) the scaled sums of a result tuple, in the entry point's order."""
    r, c = zip(*R.TRIU)
    return torch.cat((ne.cost[:, None], ne.gradient, ne.hessian[:, list(r), list(c)]), dim=1)


def random_semantics(N, seed):
    """kinds uniform in 0..3 (int64) and targets uniform in +-0.02 (float32), on the device."""
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.integers(0, 4, size=N)).cuda(),
            torch.from_numpy(rng.uniform(-0.02, 0.02, size=N).astype(np.float32)).cuda())


@functools.lru_cache(maxsize=1)
def surface_samples():
    """The most points a test here asks for, sampled from the drill's surface once."""
    return pv.sample_mesh_points(W.build_drill(), num_points=max(COUNTS), name="drill", dbpath=None,
                                 device="cuda")[0].to(torch.float32)


def near_cloud(n, seed):
    """n points within about 1 cm of the drill's surface: with targets in +-0.02 the residuals have both signs and lie on both
    sides of DELTA, so every class of pair occurs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (surface_samples()[:n] + (torch.rand((n, 3), generator=g, device="cuda") * 2 - 1) * 0.01).contiguous()


def check_sem(ne, x, v, n, inside, kinds, targets, delta, N, scale, label):
    """The five counts equal the restatement's (the decisions are single IEEE operations on the same inputs); per entry of the
    sums |got - want| <= (N + BOUND_C) 2^-53 fsum |terms|, want = fsum of the contract's terms (the count of BOUND_C is stated
    where it is defined).  Returns (worst error / bound, the counts summed over the poses)."""
    k = scale * scale / N
    got_all = packed(ne, N, scale).cpu().numpy() / k
    hess = ne.hessian.cpu().numpy()
    got_counts = torch.cat((ne.counts[:, None], ne.active, ne.outliers[:, None]), dim=1).cpu().numpy()
    worst, total = 0.0, np.zeros(S.COUNTS, dtype=np.int64)
    for b in range(x.shape[0]):
        t, counts = S.sem_terms(v[b], n[b], x[b], kinds, targets, delta, in_range=None if inside is None else inside[b])
        assert np.array_equal(got_counts[b], counts), (label, b, got_counts[b], counts)
        total += counts
        assert np.array_equal(hess[b], hess[b].T), label
        want, mag = R.fsum_columns(t), R.fsum_columns(np.abs(t))
        if np.isnan(want).any():
            assert np.array_equal(np.isnan(got_all[b]), np.isnan(want)), label
            continue
        bound = (N + S.BOUND_C) * U * mag
        err = np.abs(got_all[b] - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, b, err, bound)
    return worst, total


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
@pytest.mark.parametrize("index_f64", [True, False])
def test_degenerate_case_is_the_chamfer_kernel_bit_for_bit(caches, index_f64, mode):
    """All kinds SURFACE, all targets 0, delta = inf -- given explicitly, left out, and as NULL pointers through the C entry point:
    cost, gradient, hessian and counts of chamfer_normal_equations, bit for bit.  This pins the order of summation."""
    c = caches[(index_f64, mode)]
    for N in COUNTS:
        zeros_k, zeros_t = torch.zeros(N, dtype=torch.int64, device="cuda"), torch.zeros(N, device="cuda")
        for name, pts in clouds(c, N).items():
            for B in (1, 3):
                Wm = poses(B, seed=N + B, trans=0.005, rot=0.01)
                old = pv.chamfer_normal_equations(Wm, pts, c)
                explicit = pv.semantic_normal_equations(Wm, pts, c, semantics=zeros_k, targets=zeros_t, huber_delta=math.inf)
                left_out = pv.semantic_normal_equations(Wm, pts, c)
                for new in (explicit, left_out):
                    for f in ("cost", "gradient", "hessian", "counts"):
                        assert torch.equal(getattr(new, f), getattr(old, f)), (N, name, B, f)
                    assert new.cost.dtype == new.gradient.dtype == new.hessian.dtype == torch.float64
                    assert new.counts.dtype == new.active.dtype == new.outliers.dtype == torch.int64
                    assert new.counts.shape == (B,) and new.active.shape == (B, 3) and new.outliers.shape == (B,)
                    assert (new.active[:, 0] == N).all() and (new.active[:, 1:] == 0).all() and (new.outliers == 0).all()
                sums, counts = run_sem(c, Wm, pts)
                assert torch.equal(sums * (1e6 / N), packed(old, N)), (N, name, B)
                assert torch.equal(counts[:, 0], old.counts) and counts[:, 1:].tolist() == [[N, 0, 0, 0]] * B


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
@pytest.mark.parametrize("index_f64", [True, False])
def test_sums_and_counts_against_the_contract(caches, index_f64, mode):
    """Random kinds in 0..3, targets uniform in +-0.02, delta = 0.01, on the three clouds of test_registration_gpu and on one that
    hugs the surface.  On the latter, for N >= 64, every class of pair must occur -- SURFACE active, FREE and OCCUPIED both active
    and inactive, IGNORE, inliers and outliers -- or the inputs prove nothing."""
    c = caches[(index_f64, mode)]
    worst = 0.0
    for N in COUNTS:
        kinds, targets = random_semantics(N, seed=100 + N)
        kn, tn = kinds.cpu().numpy(), targets.cpu().numpy()
        for name, pts in dict(clouds(c, N), near=near_cloud(N, seed=14)).items():
            for B in (1, 3):
                Wm = poses(B, seed=N + B, trans=0.005, rot=0.01)
                ne = pv.semantic_normal_equations(Wm, pts, c, semantics=kinds, targets=targets, huber_delta=DELTA)
                x = transformed(Wm, pts)
                v, n, inside = cache_vn(c, x)
                w, total = check_sem(ne, x.cpu().numpy(), v, n, inside, kn, tn, DELTA, N, 1000., (N, name, B))
                worst = max(worst, w)
                if name == "near" and N >= 64:
                    per_kind = np.array([(kn == k).sum() for k in range(4)]) * B
                    assert (per_kind > 0).all()
                    assert total[1] == per_kind[0]
                    assert 0 < total[2] < per_kind[1] and 0 < total[3] < per_kind[2], (N, B, total, per_kind)
                    assert 0 < total[4] < total[1:4].sum(), (N, B, total)
    print(f"semantic sums vs contract [{mode}, index_f64={index_f64}]: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_placed_edges(caches, mode):
    """r == 0 exactly on points of each kind (targets[i] = v_i: FREE and OCCUPIED inactive, SURFACE active with zero terms) and
    a == delta exactly on a chosen pair (an inlier); one float64 step below that delta the same pair is an outlier."""
    c = caches[(True, mode)]
    N = CHUNK + 65
    pts = near_cloud(N, seed=15)
    Wm = poses(1, seed=16, trans=0.005, rot=0.01)
    kinds, targets = random_semantics(N, seed=17)
    x = transformed(Wm, pts)
    v, n, inside = cache_vn(c, x)
    kn, tn = kinds.cpu().numpy(), targets.cpu().numpy().copy()
    placed = np.concatenate([np.flatnonzero(kn == k)[:5] for k in range(4)])
    tn[placed] = v[0][placed]
    r = S.residual(v[0], tn)
    assert (r[placed] == 0.0).all()
    pick = int(np.flatnonzero((kn == 0) & (np.abs(r) > 0.002) & (np.abs(r) < 0.015))[7])
    delta = float(abs(r[pick]))
    targets = torch.from_numpy(tn).cuda()
    xs = x.cpu().numpy()
    ne = pv.semantic_normal_equations(Wm, pts, c, semantics=kinds, targets=targets, huber_delta=delta)
    _, total = check_sem(ne, xs, v, n, inside, kn, tn, delta, N, 1000., "placed")
    # the placed points: 5 SURFACE pairs active, none of the 10 one-sided ones
    without = S.sem_terms(np.delete(v[0], placed), np.delete(n[0], placed, 0), np.delete(xs[0], placed, 0), np.delete(kn, placed),
                          np.delete(tn, placed), delta)[1]
    assert total[1] == without[1] + 5 and total[2] == without[2] and total[3] == without[3] and total[4] == without[4]
    below = float(np.nextafter(delta, 0.0))
    ne2 = pv.semantic_normal_equations(Wm, pts, c, semantics=kinds, targets=targets, huber_delta=below)
    _, total2 = check_sem(ne2, xs, v, n, inside, kn, tn, below, N, 1000., "placed, one step below")
    assert total2[4] == total[4] + 1 and (total2[1:4] == total[1:4]).all()


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_a_nan_record_poisons_its_own_pose_only_and_only_through_an_active_pair(mode):
    c = build_cache(True, mode)
    centre, k = deepest_voxel_centre(c)
    cloud = W.c2_points(c, 3000, seed=41)
    cloud = cloud[(cloud - torch.tensor(centre, dtype=torch.float32, device="cuda")).norm(dim=-1) > 0.03]  # clear of the voxel
    far = torch.full((1, 3), 5.0, device="cuda")
    pts = torch.cat((cloud, far))
    N = pts.shape[0]
    Wm = torch.eye(4, device="cuda").repeat(3, 1, 1)
    Wm[0, :3, 3] = 1.0  # pose 0: everything out of range
    Wm[1, :3, 3] = torch.tensor(centre, dtype=torch.float32, device="cuda") - far[0]  # pose 1: the far point lands on the voxel
    kinds, targets = random_semantics(N, seed=42)
    targets[-1] = 0.0  # r = v < 0 at the deepest voxel: without the NaN the far point is active as FREE, inactive as OCCUPIED
    results = {}
    for kind in (pv.POINT_SURFACE, pv.POINT_FREE, pv.POINT_OCCUPIED, pv.POINT_IGNORE, 77):
        kinds[-1] = kind
        results[kind] = pv.semantic_normal_equations(Wm, pts, c, semantics=kinds, targets=targets, huber_delta=DELTA)
        assert not any(torch.isnan(t).any() for t in results[kind][:3])
    with torch.no_grad():
        c._packed[k] = float("nan")
    for kind, clean in results.items():
        kinds[-1] = kind
        ne = pv.semantic_normal_equations(Wm, pts, c, semantics=kinds, targets=targets, huber_delta=DELTA)
        if kind in (pv.POINT_IGNORE, 77):  # the pair that reads the record is inactive: nothing of it reaches a sum
            for f in FIELDS:
                assert torch.equal(getattr(ne, f), getattr(clean, f)), (kind, f)
            continue
        assert torch.isnan(ne.cost[1]) and torch.isnan(ne.gradient[1]).all() and torch.isnan(ne.hessian[1]).all()
        for b in (0, 2):
            for f in FIELDS:
                assert torch.equal(getattr(ne, f)[b], getattr(clean, f)[b]), (kind, b, f)
        assert torch.equal(ne.counts, clean.counts)
        # a NaN residual fails both comparisons: the pair is active under every kind that can be
        assert ne.active[1, kind] == clean.active[1, kind] + (1 if kind == pv.POINT_OCCUPIED else 0)
    kinds[-1] = pv.POINT_SURFACE
    res = pv.refine_poses(Wm, pts, c, iterations=2, semantics=kinds, targets=targets, huber_delta=DELTA)
    assert torch.isnan(res.cost[1]) and not torch.isnan(res.cost[[0, 2]]).any()
    assert torch.equal(res.world_to_object[1], Wm[1])  # a NaN system takes no step


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_two_calls_and_a_graph_replay_give_the_same_bits(caches, mode):
    c = caches[(True, mode)]
    N = 3 * CHUNK + 17
    pts = near_cloud(N, seed=31)
    Wm = poses(7, seed=32)
    kinds, targets = random_semantics(N, seed=33)
    kw = dict(semantics=kinds, targets=targets, huber_delta=DELTA)
    a = pv.semantic_normal_equations(Wm, pts, c, **kw)
    b = pv.semantic_normal_equations(Wm, pts, c, **kw)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not any(t.requires_grad for t in a)
    ra = pv.refine_poses(Wm, pts, c, iterations=3, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gn = pv.semantic_normal_equations(Wm, pts, c, **kw)
        gr = pv.refine_poses(Wm, pts, c, iterations=3, **kw)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for f in FIELDS:
            assert torch.equal(getattr(a, f), getattr(gn, f)), f
        for f in ("world_to_object", "cost", "initial_cost", "accepted"):
            assert torch.equal(getattr(ra, f), getattr(gr, f)), f


def test_more_poses_than_one_grid_dimension_holds(nearest):
    """The launch carries the pose in blockIdx.y (at most 65,535) and loops over the rest: B = 65,537.  The five counts of every
    pose, and the full check on the poses around the split."""
    B, N = 65537, 3
    pts = near_cloud(N, seed=3)
    Wm = poses(B, seed=5)
    kinds = torch.tensor([pv.POINT_SURFACE, pv.POINT_FREE, pv.POINT_OCCUPIED], device="cuda")
    targets = torch.tensor([0.004, 0.015, -0.015], device="cuda")
    ne = pv.semantic_normal_equations(Wm, pts, nearest, semantics=kinds, targets=targets, huber_delta=DELTA)
    x = transformed(Wm, pts)
    v, n, inside = cache_vn(nearest, x)
    kn, tn = kinds.cpu().numpy(), targets.cpu().numpy()
    want = S.sem_counts(v, kn, tn, DELTA, inside)
    got = torch.cat((ne.counts[:, None], ne.active, ne.outliers[:, None]), dim=1).cpu().numpy()
    assert np.array_equal(got, want)
    # the one-sided decisions and the branch fall both ways
    assert all(0 < want[:, e].sum() < B for e in (2, 3)) and 0 < want[:, 4].sum() < want[:, 1:4].sum()
    sel = [0, 1, 65534, 65535, 65536]
    sub = reg.SemanticNormalEquations(*(t[sel] for t in ne))
    check_sem(sub, x.cpu().numpy()[sel], v[sel], n[sel], inside[sel], kn, tn, DELTA, N, 1000., "split")


def hand_loop(c, W0, pts, iterations, evaluate, scale=1000., damping=1e-3, up=10., down=0.1):
    """refine_poses' loop through ctypes: evaluate(W32) -> raw sums (B, 28), then pvamd_pose_lm_step."""
    lib = _lib.load()
    B, N = W0.shape[0], pts.shape[0]
    w_try = W0[:, :3, :].to(torch.float64).contiguous()
    w_acc = torch.empty_like(w_try)
    sums_acc = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device="cuda")
    lam = torch.full((B,), damping, dtype=torch.float64, device="cuda")
    accepted = torch.zeros((B,), dtype=torch.int32, device="cuda")
    w_next = W0.clone()
    initial = None
    for it in range(iterations + 1):
        sums = evaluate(w_next)
        if it == 0:
            initial = sums[:, 0].clone()
        _lib.check(lib.pvamd_pose_lm_step(B, _lib.ptr(sums), int(it == 0), _lib.ptr(w_acc), _lib.ptr(sums_acc), _lib.ptr(lam),
                                          _lib.ptr(accepted), _lib.ptr(w_try), _lib.ptr(w_next), up, down, reg.LAMBDA_MIN,
                                          reg.LAMBDA_MAX, _lib.stream_ptr()), "pvamd_pose_lm_step")
    k = scale * scale / N
    return w_acc.to(torch.float32), sums_acc[:, 0] * k, initial * k, accepted.to(torch.int64)


def chamfer_sums(c, Wm, pts):
    B, N = Wm.shape[0], pts.shape[0]
    sums = torch.empty((B, _lib.REG_SUMS), dtype=torch.float64, device="cuda")
    counts = torch.empty((B,), dtype=torch.int64, device="cuda")
    scratch = _lib.scratch_buffer(_lib.chamfer_normal_eq_scratch_bytes(B, N), "cuda")
    desc = c._grid_desc()
    _lib.check(_lib.load().pvamd_chamfer_normal_eq(ctypes.byref(desc), _lib.LEAF_MODES[c.interpolation], _lib.ptr(Wm), B,
                                                   _lib.ptr(pts), N, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(scratch),
                                                   _lib.stream_ptr()), "pvamd_chamfer_normal_eq")
    return sums


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_the_loop_is_the_pieces(caches, mode):
    c = caches[(True, mode)]
    N = CHUNK + 65
    pts = near_cloud(N, seed=61)
    W0 = poses(5, seed=62, trans=0.01, rot=0.05)
    kinds, targets = random_semantics(N, seed=63)
    k8 = reg._prepare_semantics(kinds, None, pts.device)[0]
    cases = {"all three": (dict(semantics=kinds, targets=targets, huber_delta=DELTA), (k8, targets, DELTA)),
             "delta alone": (dict(huber_delta=0.003), (None, None, 0.003)),
             "kinds alone": (dict(semantics=kinds), (k8, None, math.inf))}
    for label, (kw, (ck, ct, cd)) in cases.items():
        res = pv.refine_poses(W0, pts, c, iterations=3, **kw)
        w, cost, initial, accepted = hand_loop(c, W0, pts, 3, lambda Wm: run_sem(c, Wm, pts, ck, ct, cd)[0])
        assert torch.equal(res.world_to_object[:, :3, :], w), label
        assert torch.equal(res.cost, cost) and torch.equal(res.initial_cost, initial) and torch.equal(res.accepted, accepted), label
        assert (res.cost <= res.initial_cost).all() and (res.accepted >= 1).all()
    # nothing asked for: the kernels and the bits of "Chamfer normal equations"
    res = pv.refine_poses(W0, pts, c, iterations=3)
    w, cost, initial, accepted = hand_loop(c, W0, pts, 3, lambda Wm: chamfer_sums(c, Wm, pts))
    assert torch.equal(res.world_to_object[:, :3, :], w) and torch.equal(res.cost, cost) and torch.equal(res.accepted, accepted)
    explicit = pv.refine_poses(W0, pts, c, iterations=3, semantics=torch.zeros_like(kinds), targets=torch.zeros_like(targets),
                               huber_delta=math.inf)
    for f in ("world_to_object", "cost", "initial_cost", "accepted"):
        assert torch.equal(getattr(res, f), getattr(explicit, f)), f


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_free_space_on_the_cache(caches, mode):
    """FREE points where the cache's value at every pose used exceeds one voxel diagonal: zero cost, zero gradient, a zero
    hessian, and refine_poses returns the input poses bit for bit.  The same points under poses pushed 3 cm into them: some are
    active, and the loop does not end above its start (strictly below where the start is positive)."""
    c = caches[(True, mode)]
    diag = 0.01 * math.sqrt(3.0)
    pts = W.c2_points(c, 6000, seed=81, margin=-0.03)
    W0 = poses(3, seed=82, trans=0.0005, rot=0.001)
    W0[0] = torch.eye(4, device="cuda")
    v, _, _ = cache_vn(c, transformed(W0, pts))
    pts = pts[torch.from_numpy((v > diag).all(0)).cuda()].contiguous()
    N = pts.shape[0]
    assert N > 2000
    kinds = torch.full((N,), pv.POINT_FREE, dtype=torch.int32, device="cuda")
    ne = pv.semantic_normal_equations(W0, pts, c, semantics=kinds)
    assert (ne.cost == 0).all() and (ne.gradient == 0).all() and (ne.hessian == 0).all()
    assert not any(torch.signbit(t).any() for t in ne[:3])
    assert (ne.active == 0).all() and (ne.outliers == 0).all() and (ne.counts == N).all()
    res = pv.refine_poses(W0, pts, c, iterations=4, semantics=kinds)
    assert torch.equal(res.world_to_object, W0) and (res.cost == 0).all() and (res.accepted == 1).all()
    pushed = W0.clone()
    pushed[:, :3, 3] += torch.tensor([[0.03, 0.0, 0.0], [0.0, -0.03, 0.0], [0.0, 0.0, 0.03]], device="cuda")
    start = pv.semantic_normal_equations(pushed, pts, c, semantics=kinds)
    assert (start.active[:, 1] > 0).all() and (start.active[:, [0, 2]] == 0).all()
    res = pv.refine_poses(pushed, pts, c, iterations=10, semantics=kinds)
    print(f"free space on the cache [{mode}]: N {N}, active {start.active[:, 1].tolist()}, cost {res.initial_cost.tolist()} -> "
          f"{res.cost.tolist()}")
    assert torch.equal(res.initial_cost, start.cost)
    assert (res.cost <= res.initial_cost).all()
    assert (res.cost[res.initial_cost > 0] < res.initial_cost[res.initial_cost > 0]).all()


@pytest.mark.parametrize("kind", ["mesh", "sphere"])
def test_generic_path(kind):
    obj = pv.MeshSDF(W.build_drill()) if kind == "mesh" else pv.SphereSDF(0.1)
    N, B = 700, 3
    pts = W.uniform_points_device(N, [-0.12] * 3, [0.12] * 3, 51)
    Wm = poses(B, seed=52)
    kinds, targets = random_semantics(N, seed=53)
    ne = pv.semantic_normal_equations(Wm, pts, obj, scale=10., semantics=kinds, targets=targets, huber_delta=DELTA)
    x = transformed(Wm, pts)
    v, n = obj(x)
    assert (ne.counts == N).all()
    worst, total = check_sem(ne, x.cpu().numpy(), v.float().cpu().numpy(), n.float().cpu().numpy(), None, kinds.cpu().numpy(),
                             targets.cpu().numpy(), DELTA, N, 10., kind)
    assert (total[1:] > 0).all()
    print(f"generic path [{kind}]: worst error / bound = {worst:.3g}; counts over {B} poses {total.tolist()}")
    plain = pv.semantic_normal_equations(Wm, pts, obj, scale=10.)
    old = pv.chamfer_normal_equations(Wm, pts, obj, scale=10.)
    assert torch.allclose(plain.cost, old.cost, rtol=1e-12, atol=0) and (plain.active[:, 0] == N).all()
    res = pv.refine_poses(Wm, pts, obj, iterations=2, scale=10., semantics=kinds, targets=targets, huber_delta=DELTA)
    assert (res.cost <= res.initial_cost).all() and (res.accepted >= 1).all()
    assert torch.allclose(res.initial_cost, ne.cost, rtol=1e-12, atol=0)


def test_peak_memory_has_no_per_pair_buffer(tri):
    """Above the inputs, a call at B = 64, N = 16,384 allocates its scratch, its outputs and the converted kinds (one byte a
    point, through int64 temporaries of N elements): less than one (B, N) float32 buffer."""
    B, N = 64, 16384
    pts = W.c2_points(tri, N, seed=71)
    Wm = poses(B, seed=72)
    kinds, targets = random_semantics(N, seed=73)
    kw = dict(semantics=kinds, targets=targets, huber_delta=DELTA)
    pv.semantic_normal_equations(Wm[:2], pts[:10], tri, semantics=kinds[:10], targets=targets[:10], huber_delta=DELTA)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()  # the inputs and the cache
    ne = pv.semantic_normal_equations(Wm, pts, tri, **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    allowed = _lib.semantic_normal_eq_scratch_bytes(B, N) + 3 * B * 28 * 8 + B * (5 + 36) * 8 + 4 * 8 * N + (1 << 20)
    print(f"peak extra memory {peak} B, allowed {allowed} B; one (B, N) float32 buffer would be {4 * B * N} B")
    assert peak <= allowed, (peak, allowed)
    assert 4 * B * N > allowed
    assert (ne.counts <= N).all()
