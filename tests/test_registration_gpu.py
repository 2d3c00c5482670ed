"""GPU: pv.chamfer_normal_equations / pv.refine_poses (csrc/registration.hip) against include/pvamd.h "Chamfer normal equations"
and its float64 restatement tests/registration_ref.py, on the drill cache at 0.01 m with 0.1 m padding."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
import workloads as W
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import registration as reg
from tests import registration_ref as R
from tests.test_interp_gpu import run_abi
from tests.test_min_over_points_gpu import deepest_voxel_centre, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNK = _lib.REG_CHUNK
COUNTS = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
# Loop against the restatement: the largest cost ratio - 1 over the 32 poses observed on the first GPU run was 4.2e-15 (every
# pose took the same decisions as the restatement: profiles/registration.md); ten times that is below the floor, so m = 1e-6.
LOOP_M = 1e-6
LOOP_SEED = 7


def build_cache(index_f64, interpolation):
    obj = W.build_drill()
    bb = obj.bounding_box(padding=0.1)
    if not index_f64:  # python floats: the view's index arithmetic is float32 (voxel.py)
        bb = [[float(a), float(b)] for a, b in np.asarray(bb.cpu() if torch.is_tensor(bb) else bb)]
    c = pv.CachedSDF("YcbPowerDrill", 0.01, bb, pv.MeshSDF(obj), device="cuda", cache_path=None, interpolation=interpolation)
    assert bool(c._view.index_f64) == index_f64
    return c


@pytest.fixture(scope="module")
def caches():
    return {(f64, mode): build_cache(f64, mode) for f64 in (True, False) for mode in ("nearest", "trilinear")}


@pytest.fixture(scope="module")
def tri(caches):
    return caches[(True, "trilinear")]


@pytest.fixture(scope="module")
def nearest(caches):
    return caches[(True, "nearest")]


def transformed(Wm, pts):
    """x (B, N, 3) float32 = pvamd_transform_points(W, pts) on the device."""
    B, N = Wm.shape[0], pts.shape[0]
    x = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().pvamd_transform_points(_lib.ptr(Wm), B, _lib.ptr(pts), N, _lib.ptr(x), _lib.stream_ptr()),
               "pvamd_transform_points")
    return x


def cache_vn(c, x):
    """(v, n, in_range) of the cache's own float32 query at x (B, N, 3), on the host."""
    name = "pvamd_cached_query" if c.interpolation == "nearest" else "pvamd_cached_query_interp"
    v, n, oob = run_abi(name, c._grid_desc(), x.reshape(-1, 3).contiguous())
    lead = tuple(x.shape[:-1])
    return v.reshape(lead), n.reshape(lead + (3,)), (oob == 0).reshape(lead)


def poses(B, seed, trans=0.02, rot=0.1):
    return torch.from_numpy(R.perturbed_poses(B, trans, rot, seed)).cuda()


def check_sums(ne, x, v, n, N, scale, label):
    """|got - want| <= (N + 8) 2^-53 fsum(|terms|) per entry: N - 1 roundings of a recursive sum in any fixed order, plus the few
    inside a term; want = fsum of the contract's float64 terms."""
    k = scale * scale / N
    cost, grad, hess = ne.cost.cpu().numpy(), ne.gradient.cpu().numpy(), ne.hessian.cpu().numpy()
    worst = 0.0
    for b in range(x.shape[0]):
        t = R.terms(v[b], n[b], x[b])
        want, mag = R.fsum_columns(t), R.fsum_columns(np.abs(t))
        got = np.concatenate(([cost[b]], grad[b], [hess[b][r, c] for r, c in R.TRIU])) / k
        assert np.array_equal(hess[b], hess[b].T), label
        if np.isnan(want).any():
            assert np.array_equal(np.isnan(got), np.isnan(want)), label
            continue
        bound = (N + 8) * U * mag
        err = np.abs(got - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, b, err, bound)
    return worst


def clouds(c, n):
    v = c._view
    lo = np.array([float(a) for a in v.dmax]) + 0.02
    return {"mixed": W.c2_points(c, n, seed=11), "inside": W.c2_points(c, n, seed=12, margin=-0.03),
            "outside": W.uniform_points_device(n, lo, lo + 0.2, 13)}


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
@pytest.mark.parametrize("index_f64", [True, False])
def test_sums_against_the_contract(caches, index_f64, mode):
    c = caches[(index_f64, mode)]
    worst = 0.0
    for N in COUNTS:
        for name, pts in clouds(c, N).items():
            for B in (1, 3):
                # small twists: the inside cloud stays inside, the outside cloud outside
                Wm = poses(B, seed=N + B, trans=0.005, rot=0.01)
                ne = pv.chamfer_normal_equations(Wm, pts, c)
                assert ne.cost.dtype == ne.gradient.dtype == ne.hessian.dtype == torch.float64 and ne.counts.dtype == torch.int64
                assert ne.cost.shape == (B,) and ne.gradient.shape == (B, 6) and ne.hessian.shape == (B, 6, 6)
                x = transformed(Wm, pts)
                v, n, inside = cache_vn(c, x)
                assert np.array_equal(ne.counts.cpu().numpy(), inside.sum(-1)), (N, name, B)
                if name != "mixed":
                    assert inside.all() == (name == "inside") and inside.any() == (name == "inside")
                worst = max(worst, check_sums(ne, x.cpu().numpy(), v, n, N, 1000., (N, name, B)))
    print(f"sums vs contract [{mode}, index_f64={index_f64}]: worst error / bound = {worst:.3g}")


def test_more_poses_than_one_grid_dimension_holds(nearest):
    """The launch carries the pose in blockIdx.y (at most 65,535) and loops over the rest: B = 65,537."""
    B, N = 65537, 3
    pts = W.c2_points(nearest, N, seed=3)
    Wm = poses(B, seed=5)
    ne = pv.chamfer_normal_equations(Wm, pts, nearest)
    x = transformed(Wm, pts)
    v, n, inside = cache_vn(nearest, x)
    assert np.array_equal(ne.counts.cpu().numpy(), inside.sum(-1))
    xs = x.cpu().numpy()
    # every pose's cost, and the full check on the poses around the split
    t0 = v.astype(np.float64) ** 2
    want = np.array([math.fsum(r) for r in t0]) * (1e6 / N)
    assert (np.abs(ne.cost.cpu().numpy() - want) <= (N + 8) * U * want).all()
    sel = [0, 1, 65534, 65535, 65536]
    sub = reg.ChamferNormalEquations(ne.cost[sel], ne.gradient[sel], ne.hessian[sel], ne.counts[sel])
    check_sums(sub, xs[sel], v[sel], n[sel], N, 1000., "split")


def test_cost_equals_batch_chamfer_dist(nearest):
    """Both are float64 sums of the same pairs' squared values in different orders: equal within 1 float32 ulp after the cast."""
    pts = W.c2_points(nearest, 100_000, seed=21)
    Wm = poses(5, seed=22)
    cost = pv.chamfer_normal_equations(Wm, pts, nearest).cost.float().cpu().numpy()
    ref = pv.batch_chamfer_dist(Wm, pts, obj_sdf=nearest).float().cpu().numpy()
    ulps = np.abs(cost.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print("cost vs batch_chamfer_dist, float32 ulps:", ulps)
    assert (ulps <= 1).all(), (cost, ref)


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_two_calls_and_a_graph_replay_give_the_same_bits(caches, mode):
    c = caches[(True, mode)]
    pts = W.c2_points(c, 3 * CHUNK + 17, seed=31)
    Wm = poses(7, seed=32)
    a = pv.chamfer_normal_equations(Wm, pts, c)
    b = pv.chamfer_normal_equations(Wm, pts, c)
    for f in ("cost", "gradient", "hessian", "counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    ra = pv.refine_poses(Wm, pts, c, iterations=3)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gn = pv.chamfer_normal_equations(Wm, pts, c)
        gr = pv.refine_poses(Wm, pts, c, iterations=3)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for f in ("cost", "gradient", "hessian", "counts"):
            assert torch.equal(getattr(a, f), getattr(gn, f)), f
        for f in ("world_to_object", "cost", "initial_cost", "accepted"):
            assert torch.equal(getattr(ra, f), getattr(gr, f)), f


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_a_nan_record_poisons_its_own_pose_only(mode):
    c = build_cache(True, mode)
    centre, k = deepest_voxel_centre(c)
    cloud = W.c2_points(c, 3000, seed=41)
    cloud = cloud[(cloud - torch.tensor(centre, dtype=torch.float32, device="cuda")).norm(dim=-1) > 0.03]  # clear of the voxel
    far = torch.full((1, 3), 5.0, device="cuda")
    pts = torch.cat((cloud, far))
    Wm = torch.eye(4, device="cuda").repeat(3, 1, 1)
    Wm[0, :3, 3] = 1.0  # pose 0: everything out of range
    Wm[1, :3, 3] = torch.tensor(centre, dtype=torch.float32, device="cuda") - far[0]  # pose 1: the far point lands on the voxel
    # pose 2: the identity, the cloud in and around the grid
    clean = pv.chamfer_normal_equations(Wm, pts, c)
    assert not any(torch.isnan(t).any() for t in clean[:3])
    with torch.no_grad():
        c._packed[k] = float("nan")
    ne = pv.chamfer_normal_equations(Wm, pts, c)
    assert torch.isnan(ne.cost[1]) and torch.isnan(ne.gradient[1]).all() and torch.isnan(ne.hessian[1]).all()
    for b in (0, 2):
        for f in ("cost", "gradient", "hessian"):
            assert torch.equal(getattr(ne, f)[b], getattr(clean, f)[b]), (b, f)
    assert torch.equal(ne.counts, clean.counts)
    res = pv.refine_poses(Wm, pts, c, iterations=2)
    assert torch.isnan(res.cost[1]) and not torch.isnan(res.cost[[0, 2]]).any()
    assert torch.equal(res.world_to_object[1], Wm[1])  # a NaN system takes no step


@pytest.mark.parametrize("kind", ["mesh", "sphere"])
def test_generic_path(kind):
    obj = pv.MeshSDF(W.build_drill()) if kind == "mesh" else pv.SphereSDF(0.1)
    N, B = 700, 3
    pts = W.uniform_points_device(N, [-0.15] * 3, [0.15] * 3, 51)
    Wm = poses(B, seed=52)
    ne = pv.chamfer_normal_equations(Wm, pts, obj, scale=10.)
    x = transformed(Wm, pts)
    v, n = obj(x)
    assert (ne.counts == N).all()
    worst = check_sums(ne, x.cpu().numpy(), v.float().cpu().numpy(), n.float().cpu().numpy(), N, 10., kind)
    print(f"generic path [{kind}]: worst error / bound = {worst:.3g}")
    res = pv.refine_poses(Wm, pts, obj, iterations=2, scale=10.)
    assert (res.cost <= res.initial_cost).all() and (res.accepted >= 1).all()
    assert torch.allclose(res.initial_cost, ne.cost, rtol=1e-12, atol=0)


# ---- the step kernel against the restatement ----
def run_step(cases, first, up=10., down=0.1):
    """cases: list of (LMState before, sums).  One launch; returns per case (Wacc, sums_acc, lam, accepted, Wtry, W_next)."""
    B = len(cases)
    dev = "cuda"
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sums = f(np.stack([s for _, s in cases]))
    wacc = f(np.stack([st.Wacc if st.Wacc is not None else np.full((3, 4), np.nan) for st, _ in cases]))
    sacc = f(np.stack([st.sums_acc for st, _ in cases]))
    lam = f(np.array([st.lam for st, _ in cases], dtype=np.float64))
    acc = f(np.array([st.accepted for st, _ in cases], dtype=np.int32))
    wtry = f(np.stack([st.Wtry for st, _ in cases]))
    wnext = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().pvamd_pose_lm_step(B, _lib.ptr(sums), int(first), _lib.ptr(wacc), _lib.ptr(sacc), _lib.ptr(lam),
                                              _lib.ptr(acc), _lib.ptr(wtry), _lib.ptr(wnext), up, down, R.LAMBDA_MIN, R.LAMBDA_MAX,
                                              _lib.stream_ptr()), "pvamd_pose_lm_step")
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (wacc, sacc, lam, acc, wtry, wnext)]
    return [tuple(o[b] for o in out) for b in range(B)]


def pack(s0, s1, S2):
    return np.concatenate(([s0], s1, [S2[r, c] for r, c in R.TRIU]))


def spd(kappa, rng):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    M = (Q * np.logspace(0, -math.log10(kappa), 6)) @ Q.T
    return (M + M.T) / 2


def fresh_state(rng, lam, s0=2.0):
    """An accepted state: a rigid float64 pose as Wacc = Wtry (the rotation exactly orthonormal: a signed permutation)."""
    Wm = np.zeros((3, 4))
    Wm[[0, 1, 2], rng.permutation(3)] = rng.choice([-1.0, 1.0], size=3)
    Wm[:, 3] = rng.uniform(-0.2, 0.2, size=3)
    sums = pack(s0, rng.normal(size=6), spd(10., rng))
    return R.LMState(Wtry=Wm.copy(), lam=lam, Wacc=Wm.copy(), sums_acc=sums, accepted=1)


def compare_state(got, st, label):
    wacc, sacc, lam, acc, wtry, wnext = got
    assert int(acc) == st.accepted, label
    assert float(lam) == st.lam, (label, float(lam), st.lam)
    assert same_bits(sacc, st.sums_acc), label
    assert same_bits(wacc, st.Wacc), label
    want_next = st.W_next()
    assert np.array_equal(wnext[3], [0, 0, 0, 1]), label
    assert np.array_equal(wnext[:3], wtry.astype(np.float32)), label
    return wtry, want_next


def test_step_solve_and_retraction_against_the_restatement():
    """|xi_got - xi_ref|_2 <= 64 kappa(A) 2^-53 |xi_ref|_2 (the Cholesky forward-error bound c_n kappa u, n = 6, c_n = 64 >=
    3 n^2 / 2).  The kernel does not return xi; with Wacc = [I, t] the step is read back from Wtry = [Exp(w), Exp(w) t + u]:
    w from the skew part and the angle, u = t' - Exp(w) t, both in long double, which adds a few 2^-53 of |xi| -- covered by
    testing xi through Wtry with the bound of the next paragraph as well.
    Wtry: a smooth function of xi; its rotation block moves by at most sqrt(2) |dw| and its translation by sqrt(2) |dw| |t| +
    |du|, so |Wtry_got - Wtry_ref|_F <= 2 (1 + |t|) dxi, dxi the bound above, plus 16 * 2^-53 (1 + |t|) for the retraction's own
    roundings (sin and cos within 1 to 2 ulp of libm's).  The rotation block is orthonormal within 8 * 2^-53 (checked in long
    double, so that the check adds no rounding of its own)."""
    rng = np.random.default_rng(61)
    cases = []
    for kappa in (1e1, 1e4, 1e7):
        for lam in (1e-6, 1e-3, 1.0):
            S2 = spd(kappa, rng)
            target = rng.normal(size=6)
            target *= 0.1 / np.linalg.norm(target)
            st = R.LMState(Wtry=np.hstack((np.eye(3), rng.uniform(-0.2, 0.2, size=(3, 1)))), lam=lam / 0.1)
            cases.append((st, pack(1.5, S2 @ target, S2)))
    got = run_step(cases, first=True)
    for (st, sums), g in zip(cases, got):
        R.lm_step(st, sums, True)
        A = R.damped_matrix(st.sums_acc, st.lam)
        kA = np.linalg.cond(A)
        assert kA <= 1e8, kA
        wtry, _ = compare_state(g, st, kA)
        dxi = 64 * kA * U * np.linalg.norm(st.xi)
        t = np.linalg.norm(st.Wacc[:, 3])
        tol = 2 * (1 + t) * dxi + 16 * U * (1 + t)
        err = np.linalg.norm(wtry - st.Wtry)
        print(f"kappa(A) {kA:.3g} lam {st.lam:.3g}: |Wtry - ref|_F {err:.3g} (tol {tol:.3g})")
        assert err <= tol, (kA, err, tol)
        Rl = wtry[:, :3].astype(np.longdouble)
        orth = np.abs(Rl.T @ Rl - np.eye(3, dtype=np.longdouble)).max()
        assert orth <= 8 * U, orth
        # xi itself: w from Exp(w) (skew part / sinc), u = t' - Exp(w) t
        skew = 0.5 * np.array([Rl[2, 1] - Rl[1, 2], Rl[0, 2] - Rl[2, 0], Rl[1, 0] - Rl[0, 1]])
        s = np.sqrt((skew ** 2).sum())
        w = skew * (np.arcsin(s) / s)
        u = wtry[:, 3].astype(np.longdouble) - Rl @ st.Wacc[:, 3].astype(np.longdouble)
        xi = np.concatenate((u, w)).astype(np.float64)
        exi = np.linalg.norm(xi - st.xi)
        print(f"    |xi - xi_ref|_2 {exi:.3g} (bound {dxi:.3g}, read-back slack {8 * U * (1 + t):.3g})")
        assert exi <= dxi + 8 * U * (1 + t), (exi, dxi)


def test_step_decision_paths():
    rng = np.random.default_rng(62)
    cases, labels = [], []

    def add(label, st, sums):
        cases.append((st, sums))
        labels.append(label)

    st = fresh_state(rng, 1e-3)
    add("accept", st, pack(1.0, rng.normal(size=6), spd(100., rng)))
    st = fresh_state(rng, 1e-3)
    add("reject: larger s0", st, pack(3.0, rng.normal(size=6), spd(100., rng)))
    st = fresh_state(rng, 1e-3)
    add("reject: equal s0", st, pack(2.0, rng.normal(size=6), spd(100., rng)))
    st = fresh_state(rng, 1e-3)
    add("reject: NaN s0", st, pack(math.nan, rng.normal(size=6), spd(100., rng)))
    S2 = np.zeros((6, 6))
    S2[:3, :3] = spd(10., rng)[:3, :3]
    s1 = np.concatenate((rng.normal(size=3), np.zeros(3)))
    st = fresh_state(rng, 1e-3)
    add("unobserved axes", st, pack(1.0, s1, S2))
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    S2 = (Q * np.array([1.0, 1.0, 1.0, 1.0, 1.0, -5.0])) @ Q.T
    st = fresh_state(rng, 1e-3)
    add("failed pivot: indefinite", st, pack(1.0, rng.normal(size=6), (S2 + S2.T) / 2))
    S2 = spd(10., rng)
    S2[1, 4] = S2[4, 1] = math.nan
    st = fresh_state(rng, 1e-3)
    add("failed pivot: NaN entry", st, pack(1.0, rng.normal(size=6), S2))
    st = fresh_state(rng, 1e-3)
    st.Wtry[0, 1] = st.Wacc[0, 1] = -0.0
    add("S1 = 0", st, pack(1.0, np.zeros(6), spd(10., rng)))
    st = fresh_state(rng, R.LAMBDA_MIN)
    add("lambda at its minimum", st, pack(1.0, rng.normal(size=6), spd(10., rng)))
    st = fresh_state(rng, R.LAMBDA_MAX)
    add("lambda at its maximum", st, pack(3.0, rng.normal(size=6), spd(10., rng)))
    st = fresh_state(rng, R.LAMBDA_MAX)
    st.sums_acc = pack(2.0, rng.normal(size=6), -1e13 * np.eye(6))
    add("failed pivot at the maximum", st, pack(3.0, rng.normal(size=6), spd(10., rng)))
    # the trial pose differs from the accepted one, as in the loop
    for st, _ in cases:
        st.Wtry = R.retract(st.Wacc, 0.01 * rng.normal(size=6))
    cases[labels.index("S1 = 0")][0].Wtry[0, 1] = -0.0

    got = run_step(cases, first=False)
    for label, (st, sums), g in zip(labels, cases, got):
        before = st.accepted
        R.lm_step(st, sums, False)
        wtry, _ = compare_state(g, st, label)
        if np.all(st.xi == 0.0):
            assert same_bits(wtry, g[0]), label  # Wtry is Wacc bit for bit
            assert same_bits(wtry, st.Wtry), label
        else:
            assert np.allclose(wtry, st.Wtry, rtol=0, atol=1e-9), label
        if label == "unobserved axes":
            assert st.accepted == before + 1
            # the unobserved twist components are exactly zero: the rotation block of Wtry is Wacc's
            assert np.all(st.xi[3:] == 0.0) and np.any(st.xi[:3] != 0.0)
            assert same_bits(wtry[:, :3], g[0][:, :3]), label
        if label.startswith("reject"):
            assert st.accepted == before
        if label.startswith("failed pivot"):
            assert np.all(st.xi == 0.0)
    assert cases[labels.index("S1 = 0")][0].accepted == 2
    # first = 1 accepts whatever the stored sums hold
    st = R.LMState(Wtry=np.hstack((np.eye(3), np.zeros((3, 1)))), lam=1e-3)
    sums = pack(5.0, rng.normal(size=6), spd(10., rng))
    g = run_step([(st, sums)], first=True)[0]
    R.lm_step(st, sums, True)
    compare_state(g, st, "first")


# ---- the loop ----
def test_stationary_start_keeps_its_pose_bit_for_bit():
    r = 0.125
    pts = torch.cat((r * torch.eye(3), -r * torch.eye(3))).cuda()
    for dtype in (torch.float32, torch.float64):
        Wm = torch.eye(4, dtype=dtype, device="cuda").repeat(2, 1, 1)
        res = pv.refine_poses(Wm, pts, pv.SphereSDF(r), iterations=4)
        assert res.world_to_object.dtype == dtype and res.world_to_object.device == Wm.device
        assert torch.equal(res.world_to_object, Wm)
        assert (res.cost == 0).all() and (res.initial_cost == 0).all() and (res.accepted == 1).all()
    res = pv.refine_poses(torch.eye(4).repeat(2, 1, 1), pts.cpu(), pv.SphereSDF(r), iterations=1)
    assert res.world_to_object.device.type == "cpu" and res.world_to_object.dtype == torch.float32
    assert res.cost.dtype == res.initial_cost.dtype == torch.float64 and res.accepted.dtype == torch.int64


@pytest.fixture(scope="module")
def loop_setup(tri):
    pts = pv.sample_mesh_points(W.build_drill(), num_points=2000, name="drill", dbpath=None, device="cuda")[0]
    pts = pts.to(torch.float32).contiguous()
    W0 = torch.from_numpy(R.perturbed_poses(32, 0.01, math.radians(3.0), seed=LOOP_SEED)).cuda()
    return pts, W0


def test_loop_properties(tri, nearest, loop_setup):
    pts, W0 = loop_setup
    for c in (tri, nearest):
        res = pv.refine_poses(W0, pts, c, iterations=10)
        assert (res.cost <= res.initial_cost).all() and (res.accepted >= 1).all() and (res.accepted <= 11).all()
        assert res.world_to_object.dtype == torch.float32 and res.world_to_object.is_cuda
        assert torch.equal(res.world_to_object[:, 3], torch.tensor([0., 0., 0., 1.], device="cuda").expand(32, 4))
        # the returned pose has the returned cost
        again = pv.chamfer_normal_equations(res.world_to_object, pts, c)
        assert torch.equal(again.cost, res.cost)
        assert torch.equal(pv.chamfer_normal_equations(W0, pts, c).cost, res.initial_cost)
    res64 = pv.refine_poses(W0.double().cpu(), pts, tri, iterations=2)
    assert res64.world_to_object.dtype == torch.float64 and res64.world_to_object.device.type == "cpu"


def test_loop_against_the_restatement_and_usefulness(tri, loop_setup):
    """32 poses perturbed by <= 1 cm / 3 degrees around the identity, 2000 surface samples of the drill, trilinear cache, 10
    iterations.  The restatement runs its own loop on (v, n) fetched from the device query at its own trial poses; per pose the
    two final costs agree within LOOP_M either way.  Usefulness, with its bar taken from the inputs: every pose ends strictly
    below its initial cost, and at least 30 of 32 below twice the cost of the unperturbed identity pose.  The restatement alone
    stays within that cap for LOOP_SEED (asserted below on its own costs; confirmed on the first GPU run,
    profiles/registration.md)."""
    pts, W0 = loop_setup
    N = pts.shape[0]

    def evaluate(W32):
        Wm = torch.from_numpy(np.ascontiguousarray(W32)).cuda()
        x = transformed(Wm, pts)
        v, n, _ = cache_vn(tri, x)
        xs = x.cpu().numpy()
        return np.stack([R.raw_sums(v[b], n[b], xs[b]) for b in range(len(W32))])

    states, initial = R.refine(evaluate, W0.cpu().numpy(), iterations=10)
    k = 1e6 / N
    ref_cost = np.array([s.sums_acc[0] for s in states]) * k
    res = pv.refine_poses(W0, pts, tri, iterations=10)
    cost, init = res.cost.cpu().numpy(), res.initial_cost.cpu().numpy()
    ident = float(pv.chamfer_normal_equations(torch.eye(4, device="cuda")[None], pts, tri).cost[0])
    spread = max((cost / ref_cost).max(), (ref_cost / cost).max()) - 1
    print(f"loop vs restatement: largest cost ratio - 1 = {spread:.3g}; accepted gpu {res.accepted.cpu().numpy().tolist()} "
          f"ref {[s.accepted for s in states]}")
    print(f"identity cost {ident:.6g}; initial {init.min():.4g} .. {init.max():.4g}; final {cost.min():.6g} .. {cost.max():.6g}; "
          f"below 2 x identity: gpu {(cost < 2 * ident).sum()} ref {(ref_cost < 2 * ident).sum()} of 32")
    assert np.allclose(init, initial * k, rtol=1e-12, atol=0)
    assert (cost <= ref_cost * (1 + LOOP_M)).all() and (ref_cost <= cost * (1 + LOOP_M)).all(), (cost, ref_cost)
    assert (ref_cost < initial * k).all() and (ref_cost < 2 * ident).sum() >= 30
    assert (cost < init).all()
    assert (cost < 2 * ident).sum() >= 30


def test_peak_memory_has_no_per_pair_buffer(tri):
    B, N = 1024, 16384
    pts = W.c2_points(tri, N, seed=71)
    Wm = poses(B, seed=72)
    pv.refine_poses(Wm[:2], pts[:10], tri, iterations=1)  # descriptor and code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()  # the inputs and the cache
    res = pv.refine_poses(Wm, pts, tri, iterations=3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    allowed = _lib.chamfer_normal_eq_scratch_bytes(B, N) + B * (2 * 28 + 2 * 12 + 1) * 8 + B * 4 + B * 64 + (1 << 20)
    print(f"peak extra memory {peak} B, allowed {allowed} B; one (B, N) float32 buffer would be {4 * B * N} B")
    assert peak <= allowed, (peak, allowed)
    assert 4 * B * N > allowed
    assert (res.cost <= res.initial_cost).all()
