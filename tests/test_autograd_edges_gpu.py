"""-m gpu: the autograd backward (csrc/backward.hip) at the forward's decision edges, against the decision-conditioned float64
VJP (oracle/conditioned_vjp.py) -- nothing filtered out.

Inputs sit exactly on and a few ulp around range faces, surface-box faces and half-voxel planes, on exact and random rigid
transforms over 8 and 64 DISTINCT leaves, with exact ties, at the launch shapes of bwd_plan (1024 points per chunk, about
2048 workgroups).  Three kinds of comparison:
  1. float32 kernels: |got - want| <= c 2^-24 (n_chain + 8) sum|term|  (n_chain: the longest sequential accumulation the
     kernel does for that output -- A for dpoints, nchunks + 14 for dtf);
  2. float64 kernels: the same bound at 2^-53 (a dropped or double-counted pair shows even in a sum over 300k points);
  3. impulse upstreams: one (or two) non-zero pairs; everything else must be EXACTLY zero.
A disagreement of any decision (in / out, voxel, active axis, leaf) is an O(1) error and fails all of them.

C = 4: each term is a product of at most ~16 rounded operations of the kernel (x is the forward's own, exact here), each
contributing at most 1 ulp relative to the term's magnitude, which the "+ 8" covers twice over at c = 4; every accumulation step
adds at most one ulp of the running sum of magnitudes.  So the bound is a worst case, not a statistical one, and cannot flake."""
import itertools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import conditioned_vjp as cv
from oracle import oracle
from pytorch_volumetric_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu

C = 4.0
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
NPT = {torch.float32: np.float32, torch.float64: np.float64}
CHUNK = 1024  # points per backward workgroup (backward.hip kBwdChunk)


def nchunks(P):
    return max(1, -(-P // CHUNK))


def assert_bound(got, want, mag, dtype, n_chain, what):
    ok, worst, i = cv.within_bound(got, want, mag, UNIT[dtype], n_chain, c=C)
    g, w = got.detach().reshape(-1)[i].item(), want.reshape(-1)[i].item()
    assert ok, f"{what}: worst |got - want| / bound = {worst:.3g} at flat index {i} (got {g!r}, want {w!r})"


# ---------------------------------------------------------------- input sets
def ulps(v, k, dtype):
    out = np.asarray(v, dtype).copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.asarray(np.inf if k > 0 else -np.inf, dtype))
    return out


def edge_points(og, dtype, seed, n_random=400, rep=6):
    """Leaf-frame points of `dtype` (np) on and around every decision boundary of the oracle grid og: range faces (+-2 ulp),
    surface-box faces (+-1 ulp, with another axis out of range), half-voxel planes (+-1 ulp), edges and corners of the range
    (out on 1, 2, 3 axes), and a random mix over the range inflated by 20 %."""
    rng = np.random.default_rng(seed)
    c = og.c
    f64 = dtype == np.float64
    lo, hi = np.array(c.dmin[:]), np.array(c.dmax[:])
    bblo = np.array(c.dbb_min[:] if f64 else c.bb_min[:], np.float64)
    bbhi = np.array(c.dbb_max[:] if f64 else c.bb_max[:], np.float64)
    res, span = np.array(c.dres[:]), hi - lo

    def inside(n):
        return rng.uniform(lo, hi, (n, 3))

    def outside(n, d):
        below = rng.random(n) < 0.5
        return np.where(below, lo[d] - rng.uniform(1e-3, 0.1, n) * span[d], hi[d] + rng.uniform(1e-3, 0.1, n) * span[d])

    pts = []
    for d in range(3):
        for face in (lo[d], hi[d]):
            for k in range(-2, 3):
                p = inside(rep)
                p[:, d] = ulps(face, k, dtype)
                pts.append(p)
        e = (d + 1) % 3
        for face in (bblo[d], bbhi[d]):
            for k in (-1, 0, 1):
                p = inside(rep)
                p[:, d] = ulps(face, k, dtype)
                p[:, e] = outside(rep, e)
                pts.append(p)
        for kk in rng.choice(c.shape[d] - 1, size=3, replace=False):
            plane = lo[d] + (kk + 0.5) * res[d]
            for k in (-1, 0, 1):
                p = inside(rep)
                p[:, d] = ulps(plane, k, dtype)
                pts.append(p)
    for axes in itertools.chain.from_iterable(itertools.combinations(range(3), n) for n in (1, 2, 3)):
        p = inside(2 * rep)
        for d in axes:
            pick = rng.integers(0, 3, len(p))
            p[:, d] = np.where(pick == 0, ulps(lo[d], -1, dtype), np.where(pick == 1, ulps(hi[d], 1, dtype), outside(len(p), d)))
        pts.append(p)
    pts.append(rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (n_random, 3)))
    return np.concatenate(pts).astype(dtype)


def upstreams(kind, shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    wv = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype) if kind in ("val", "both") else None
    wg = torch.randn(shape + (3,), generator=g, dtype=torch.float64).to(dtype) if kind in ("grad", "both") else None
    return wv, wg


def loss_of(val, grad, wv, wg):
    out = 0
    if wv is not None:
        out = out + (val * wv.to(val.device).reshape(val.shape)).sum()
    if wg is not None:
        out = out + (grad * wg.to(grad.device).reshape(grad.shape)).sum()
    return out


# ---------------------------------------------------------------- cached
@pytest.fixture(scope="module")
def caches():
    from tests.test_cached_gpu import make_cached
    return {"f64": make_cached(f64=True), "f32": make_cached(f64=False),
            "f64_pad0": make_cached(padding=0.0, f64=True), "f32_pad0": make_cached(padding=0.0, f64=False)}


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["f64", "f32", "f64_pad0", "f32_pad0"])
def test_cached_backward_at_decision_edges(caches, kind, dtype, upstream):
    c = caches[kind]
    og = H.oracle_grid_from_cached(c)
    pts = edge_points(og, NPT[dtype], seed=1)
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (P,), dtype, seed=2)
    p = torch.from_numpy(pts).cuda().requires_grad_()
    val, grad = c(p)
    (dp,) = torch.autograd.grad(loss_of(val, grad, wv, wg), p)
    r = cv.cached_vjp(og, pts, wv, wg)
    oob = r["oob"]
    assert int(oob.sum()) > 100 and int((~oob).sum()) > 100
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], dtype, 0, f"cached {kind} dpoints")
    assert torch.equal(dp[~oob.cuda()], torch.zeros_like(dp[~oob.cuda()]))


# ---------------------------------------------------------------- composed: distinct leaves
LATTICE = 0.25


def leaf_spec(s, seed):
    """Leaf s: an analytic ellipsoid grid around its own origin, with its own resolution, padding and index dtype."""
    rng = np.random.default_rng(seed * 1000 + s)
    h = rng.uniform(0.04, 0.08, 3)
    bb = np.stack((-h + rng.uniform(-0.01, 0.01, 3), h + rng.uniform(-0.01, 0.01, 3)), axis=1)
    centre = bb.mean(axis=1) + rng.uniform(-0.01, 0.01, 3)
    radii = (bb[:, 1] - bb[:, 0]) / 2 * rng.uniform(0.6, 0.9, 3)
    return dict(gt=H.AnalyticEllipsoidSDF(centre, radii, bb), res=float(rng.choice([0.01, 0.0125, 0.02])),
                pad=float(rng.choice([0.0, 0.01, 0.03])), f64=bool(s % 2 == 0))


def build_leaves(S, seed=0):
    leaves = []
    for s in range(S):
        sp = leaf_spec(s, seed)
        rng = H.padded_range(sp["gt"].bb.numpy(), sp["pad"], as_numpy=sp["f64"])
        leaves.append(pv.CachedSDF(f"leaf{s}", sp["res"], rng, sp["gt"], device="cuda", cache_path=None))
    return leaves


@pytest.fixture(scope="module")
def leaves64():
    return build_leaves(64)


def lattice_centre(s):
    return (np.array([s % 4, (s // 4) % 4, (s // 16) % 4], np.float64) - 1.5) * LATTICE


def transforms(S, A, kind, dtype, seed):
    """(S*A, 4, 4) obj->leaf, leaf-major: leaf s sits at a lattice point of the object frame.  "exact": signed axis permutations
    and translations by binary fractions (the boundary points land exactly on the leaf-frame faces); "random": random rotations
    and jittered translations."""
    g = np.random.default_rng(seed)
    m = np.zeros((S * A, 4, 4), np.float64)
    m[:, 3, 3] = 1
    for s in range(S):
        for a in range(A):
            if kind == "exact":
                R = np.eye(3)[g.permutation(3)] * g.choice([-1.0, 1.0], 3)[:, None]
                cen = lattice_centre(s) + g.integers(-2, 3, 3) / 64
            else:
                q, r = np.linalg.qr(g.normal(size=(3, 3)))
                R = q * np.sign(np.diag(r))[None, :]
                cen = lattice_centre(s) + g.uniform(-0.02, 0.02, 3)
            if np.linalg.det(R) < 0:  # a rotation, not a reflection (only rigid stacks take the fused path with gradients)
                R[2] = -R[2]
            m[s * A + a, :3, :3] = R
            m[s * A + a, :3, 3] = -R @ cen
    return torch.from_numpy(m).to(dtype)


def object_points(ogs, m, A, dtype, seed, per_leaf=None, nudge=True):
    """Each leaf's edge points, taken to the object frame through one of its configurations (float64 inverse, rounded to
    `dtype`; random transforms: nudged by up to 2 ulp), so that they land on / around that leaf's faces in its own frame."""
    rng = np.random.default_rng(seed)
    out = []
    mm = m.double().numpy()
    for s, og in enumerate(ogs):
        x = edge_points(og, np.float64 if dtype == torch.float64 else np.float32, seed + s, n_random=60, rep=2)
        if per_leaf is not None:
            x = x[rng.permutation(len(x))[:per_leaf]]
        M = mm[s * A + (s % A)]
        p = ((x.astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(NPT[dtype])
        if nudge:
            k = rng.integers(-2, 3, p.shape)
            for kk in (-2, -1, 1, 2):
                p = np.where(k == kk, ulps(p, kk, NPT[dtype]), p)
        out.append(p)
    return np.concatenate(out)


def run_composed(comp, m, pts_t, batch_dim, wv, wg):
    mm = m.cuda().requires_grad_()
    comp.set_transforms(mm, batch_dim=batch_dim)
    p = pts_t.cuda().requires_grad_()
    val, grad = comp(p)
    assert val.grad_fn is not None
    dp, dm = torch.autograd.grad(loss_of(val, grad, wv, wg), (p, mm))
    return dp.reshape(-1, 3), dm


def check_composed(dp, dm, r, A, P, dtype, what):
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], dtype, A, f"{what} dpoints")
    assert_bound(dm, r["dtf"], r["dtf_mag"], dtype, nchunks(P) + 14, f"{what} dtf")
    assert torch.equal(dm[:, 3], torch.zeros_like(dm[:, 3])), f"{what}: row 3 of dtf"


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tkind", ["exact", "random"])
def test_composed_8_distinct_leaves_with_a_tie(leaves64, tkind, dtype, upstream):
    """S = 8 (leaf 7 is leaf 2 again, under the same transforms: an exact tie the first leaf must win), batch_dim = (2, 3),
    points shaped (2, N, 3)."""
    S, batch = 8, (2, 3)
    A = math.prod(batch)
    leaves = leaves64[:7] + [leaves64[2]]
    ogs = [H.oracle_grid_from_cached(c) for c in leaves]
    m = transforms(S, A, tkind, dtype, seed=3)
    m[7 * A:8 * A] = m[2 * A:3 * A]
    pts = object_points(ogs[:7], m, A, dtype, seed=4, nudge=tkind == "random")
    pts = pts[:len(pts) // 2 * 2]
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (A, P), dtype, seed=5)
    comp = pv.ComposedSDF(leaves, None)
    dp, dm = run_composed(comp, m, torch.from_numpy(pts).reshape(2, P // 2, 3), batch, wv, wg)
    r = cv.composed_vjp(ogs, m.numpy(), A, pts, wv, wg)
    won = set(r["leaf"].reshape(-1).tolist())
    assert 2 in won and 7 not in won and len(won) == 7
    assert torch.equal(dm[7 * A:8 * A], torch.zeros_like(dm[7 * A:8 * A]))  # the tie went to leaf 2
    check_composed(dp, dm, r, A, P, dtype, f"S=8 {tkind}")


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tkind", ["exact", "random"])
def test_composed_64_distinct_leaves_one_configuration(leaves64, tkind, dtype, upstream):
    """S = 64 (present bit 63, LDS slot 63), tsf_batch None: one configuration, one split, dpoints written directly.
    Regression (with the 8-leaf test): a value-only upstream once put NaN into dtf for pairs out of range but inside the
    surface box (|d| = 0, n = 0 / 0: a padding-0 leaf whose voxel range ends short of its box), where torch gives 0."""
    S, A = 64, 1
    ogs = [H.oracle_grid_from_cached(c) for c in leaves64]
    m = transforms(S, A, tkind, dtype, seed=6)
    pts = object_points(ogs, m, A, dtype, seed=7, per_leaf=150, nudge=tkind == "random")
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (P,), dtype, seed=8)
    comp = pv.ComposedSDF(leaves64, None)
    dp, dm = run_composed(comp, m, torch.from_numpy(pts), None, wv, wg)
    r = cv.composed_vjp(ogs, m.numpy(), A, pts, wv, wg)
    assert bool((r["leaf"] == 63).any()) and len(set(r["leaf"].reshape(-1).tolist())) == 64
    check_composed(dp, dm, r, A, P, dtype, f"S=64 {tkind}")


# ---------------------------------------------------------------- launch shapes (bwd_plan)
@pytest.mark.parametrize("P", [0, 1, 63, 65, 1023, 1025, 3089])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_partial_chunks(leaves64, P, dtype):
    S, A = 8, 6
    leaves = leaves64[8:16]
    ogs = [H.oracle_grid_from_cached(c) for c in leaves]
    m = transforms(S, A, "random", dtype, seed=9)
    rng = np.random.default_rng(11)
    pool = object_points(ogs, m, A, dtype, seed=10)
    pool = np.concatenate((pool, rng.uniform(-0.55, 0.55, (max(0, P - len(pool)), 3)).astype(NPT[dtype])))
    pts = pool[rng.permutation(len(pool))[:P]]
    wv, wg = upstreams("both", (A, P), dtype, seed=12)
    comp = pv.ComposedSDF(leaves, None)
    dp, dm = run_composed(comp, m, torch.from_numpy(pts), (A,), wv, wg)
    assert dp.shape == (P, 3) and dm.shape == (S * A, 4, 4)
    if P == 0:
        assert torch.equal(dm, torch.zeros_like(dm))
        return
    r = cv.composed_vjp(ogs, m.numpy(), A, pts, wv, wg)
    check_composed(dp, dm, r, A, P, dtype, f"P={P}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_64_leaves_8_splits(leaves64, dtype):
    """S = 64, A = 8, P = 5000: five chunks (the last partial), eight splits of one configuration."""
    S, A, P = 64, 8, 5000
    ogs = [H.oracle_grid_from_cached(c) for c in leaves64]
    m = transforms(S, A, "random", dtype, seed=13)
    pool = object_points(ogs, m, A, dtype, seed=14, per_leaf=100)
    pts = pool[np.random.default_rng(15).permutation(len(pool))[:P]]
    wv, wg = upstreams("both", (A, P), dtype, seed=16)
    dp, dm = run_composed(pv.ComposedSDF(leaves64, None), m, torch.from_numpy(pts), (A,), wv, wg)
    r = cv.composed_vjp(ogs, m.numpy(), A, pts, wv, wg)
    assert bool((r["leaf"] == 63).any())
    check_composed(dp, dm, r, A, P, dtype, "S=64 A=8 P=5000")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_uneven_splits_300k(leaves64, dtype):
    """S = 8, A = 20, P = 300,017: 293 chunks (the last partial), aper = 3, seven splits, the last of 2 configurations."""
    S, A, P = 8, 20, 300_017
    leaves = leaves64[16:24]
    ogs = [H.oracle_grid_from_cached(c) for c in leaves]
    m = transforms(S, A, "random", dtype, seed=17)
    pool = object_points(ogs, m, A, dtype, seed=18)
    rng = np.random.default_rng(19)
    far = rng.uniform(-0.55, 0.55, (P - len(pool), 3)).astype(NPT[dtype])
    pts = np.concatenate((pool, far))[rng.permutation(P)]
    wv, wg = upstreams("both", (A, P), dtype, seed=20)
    dp, dm = run_composed(pv.ComposedSDF(leaves, None), m, torch.from_numpy(pts), (A,), wv, wg)
    r = cv.composed_vjp(ogs, m.numpy(), A, pts, wv, wg)
    check_composed(dp, dm, r, A, P, dtype, "S=8 A=20 P=300017")


def test_composed_65_leaves_raise(leaves64):
    comp = pv.ComposedSDF(leaves64 + [leaves64[0]], None)
    comp.set_transforms(torch.eye(4).repeat(65, 1, 1).requires_grad_())
    with pytest.raises(_lib.PvamdError):
        comp(torch.zeros(10, 3, device="cuda"))


# ---------------------------------------------------------------- impulses
IMPULSE_P = 300_017


@pytest.fixture(scope="module", params=[torch.float32, torch.float64], ids=["f32", "f64"])
def impulse_setup(request, leaves64):
    """S = 64, A = 20, P = 300,017 (aper = 3): points far outside every leaf (their box branch has |d| > 0, so a zero upstream
    makes exact zero terms -- a pair out of range but inside the box has n = 0 / 0, and NaN x 0 reaches dtf there as it does
    in torch), and at the swept indices a point outside the corner leaf 0 (or 63) on all three axes, so that leaf wins there
    for every configuration."""
    dtype = request.param
    S, A, P = 64, 20, IMPULSE_P
    m = transforms(S, A, "random", dtype, seed=21)
    rng = np.random.default_rng(22)
    base = rng.uniform(-0.9, 0.9, (3 * P, 3))
    base = base[np.abs(base).max(axis=1) > 0.66][:P]  # > 0.28 from every lattice centre: outside every leaf's range and box
    return dtype, m, base


SWEEP_P = [0, 63, 64, 255, 256, 1023, 1024, IMPULSE_P - 1]
SWEEP_A = [0, 2, 3, 19]  # 0, aper - 1, aper, A - 1 for aper = 3


def wave_partner(p):
    """another point index of the same wave (64 consecutive indices) as p"""
    return p + 1 if (p + 1) % 64 and p + 1 < IMPULSE_P else p - 1


@pytest.mark.parametrize("winner", [0, 63])
def test_impulse_upstreams_hit_exactly_one_slot(leaves64, impulse_setup, winner):
    dtype, m, base = impulse_setup
    S, A, P = 64, 20, IMPULSE_P
    other = 63 - winner
    pts = base.copy()
    corner = lambda s: lattice_centre(s) + np.sign(lattice_centre(s)) * 0.16
    for p in SWEEP_P:
        pts[p] = corner(winner)
        pts[wave_partner(p)] = corner(other)
    pts = pts.astype(NPT[dtype])
    ogs = [H.oracle_grid_from_cached(c) for c in leaves64]
    comp = pv.ComposedSDF(leaves64, None)
    mm = m.cuda().requires_grad_()
    comp.set_transforms(mm, batch_dim=(A,))
    pt = torch.from_numpy(pts).cuda().requires_grad_()
    val, grad = comp(pt)
    g = torch.Generator().manual_seed(23)
    for p in SWEEP_P:
        q = wave_partner(p)
        for a in SWEEP_A:
            for pairs in ([p], [p, q]):
                dv = torch.zeros(A, P, dtype=dtype)
                dg = torch.zeros(A, P, 3, dtype=dtype)
                for i in pairs:
                    dv[a, i] = torch.randn((), generator=g, dtype=torch.float64).to(dtype)
                    dg[a, i] = torch.randn(3, generator=g, dtype=torch.float64).to(dtype)
                dp, dm = torch.autograd.grad(loss_of(val, grad, dv, dg), (pt, mm), retain_graph=True)
                sub = pts[pairs]
                r = cv.composed_vjp(ogs, m.numpy(), A, sub, dv[:, pairs], dg[:, pairs])
                want_leaf = [winner, other][:len(pairs)]
                assert r["leaf"][a].tolist() == want_leaf, (p, a, r["leaf"][a])
                slots = [s * A + a for s in want_leaf]
                rest = torch.ones(S * A, dtype=torch.bool)
                rest[slots] = False
                what = f"impulse p*={p} a*={a} pairs={pairs}"
                assert torch.equal(dm[rest.cuda()], torch.zeros_like(dm[rest.cuda()])), what
                assert_bound(dm[slots], r["dtf"][slots], r["dtf_mag"][slots], dtype, 0, what + " dtf")
                assert bool((dm[slots, :3].abs().sum((1, 2)) > 0).all()), what
                rows = torch.zeros(P, dtype=torch.bool)
                rows[pairs] = True
                assert torch.equal(dp[~rows.cuda()], torch.zeros_like(dp[~rows.cuda()])), what
                assert_bound(dp[pairs], r["dpoints"], r["dpoints_mag"], dtype, 0, what + " dpoints")


# ---------------------------------------------------------------- chamfer
@pytest.mark.parametrize("N,B", [(1, 1), (1, 40), (1023, 6), (1023, 40), (3001, 1), (3001, 6)])
def test_grid_chamfer_gradients_to_pose_and_points(caches, N, B):
    c = caches["f64"]
    og = H.oracle_grid_from_cached(c)
    scale = 1000.0
    W = H.random_rigid(B, seed=24, trans=0.05)
    x = edge_points(og, np.float32, seed=25, n_random=max(400, N))
    x = x[np.random.default_rng(26).permutation(len(x))[:N]]
    assert x.shape == (N, 3)
    # world points whose object-frame images under the first transform are the edge points; the others see them rotated
    Wi = W[0].double().numpy()
    pts = ((x.astype(np.float64) - Wi[:3, 3]) @ Wi[:3, :3]).astype(np.float32)
    w = torch.randn(B, generator=torch.Generator().manual_seed(27)).double()  # float32 values: the output is float32
    Wg = W.cuda().requires_grad_()
    pg = torch.from_numpy(pts).cuda().requires_grad_()
    err = pv.batch_chamfer_dist(Wg, pg, obj_sdf=c, scale=scale)
    assert err.grad_fn is not None
    dW, dp = torch.autograd.grad((err.double() * w.cuda()).sum(), (Wg, pg))
    r = cv.chamfer_vjp(og, W.numpy(), pts, scale, w / N)
    assert torch.equal(dW[:, 3], torch.zeros_like(dW[:, 3]))
    assert_bound(dW, r["dW"], r["dW_mag"], torch.float32, nchunks(N) + 14, f"chamfer N={N} B={B} dW")
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], torch.float32, B, f"chamfer N={N} B={B} dpoints")


# ---------------------------------------------------------------- robot: composed dpoints
def test_robot_dpoints_grad_only_loss():
    import workloads as W
    robot = W.build_c4()
    A, P = 20, 20000
    q = W.c4_joint_configs(A, seed=3).cuda()
    robot.set_joint_configuration(q)
    pts = W.c4_points(P, seed=4)
    wg = torch.randn(A, P, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64).float()
    p = pts.clone().requires_grad_()
    _, grad = robot(p)
    assert grad.grad_fn is not None
    (dp,) = torch.autograd.grad((grad * wg.cuda()).sum(), p)
    stack = robot.sdf._tf_matrix.detach().cpu()
    ogs = [H.oracle_grid_from_cached(c) for c in robot.sdf.sdfs]
    r = cv.composed_vjp(ogs, stack.numpy(), A, pts.cpu().numpy(), None, wg)
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], torch.float32, A, "robot dpoints")


# ---------------------------------------------------------------- in-place writes between forward and backward
def test_inplace_write_after_forward_cached(caches):
    """float32 contiguous device points are used where they are: the backward must differentiate at what the forward saw."""
    c = caches["f64"]
    pts = torch.from_numpy(edge_points(H.oracle_grid_from_cached(c), np.float32, seed=28)).cuda()
    p = pts.clone().requires_grad_()
    val, grad = c(p)
    with torch.no_grad():
        p.add_(0.05)
    (got,) = torch.autograd.grad(val.sum() + grad.sum(), p)
    q = pts.clone().requires_grad_()
    v2, g2 = c(q)
    (want,) = torch.autograd.grad(v2.sum() + g2.sum(), q)
    assert torch.equal(got, want)


@pytest.mark.parametrize("what", ["points", "transforms"])
def test_inplace_write_after_forward_composed_raises(leaves64, what):
    S, A = 8, 3
    m = transforms(S, A, "random", torch.float32, seed=29).cuda().requires_grad_()
    comp = pv.ComposedSDF(leaves64[:S], None)
    comp.set_transforms(m, batch_dim=(A,))
    p = (torch.rand(500, 3, generator=torch.Generator().manual_seed(30)) - 0.5).cuda().requires_grad_()
    val, grad = comp(p)
    with torch.no_grad():
        (p if what == "points" else m).add_(0.05)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(val.sum() + grad.sum(), (p, m))


@pytest.mark.parametrize("what", ["points", "transforms"])
def test_inplace_write_after_forward_chamfer_raises(caches, what):
    c = caches["f64"]
    W = H.random_rigid(4, seed=31, trans=0.05).cuda().requires_grad_()
    p = torch.from_numpy(edge_points(H.oracle_grid_from_cached(c), np.float32, seed=32)).cuda().requires_grad_()
    err = pv.batch_chamfer_dist(W, p, obj_sdf=c, scale=1000.0)
    with torch.no_grad():
        (p if what == "points" else W).add_(0.05)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(err.sum(), (W, p))
