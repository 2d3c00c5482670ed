"""-m gpu: the TRILINEAR backward (interp_cell / interp_fraction_vjp of csrc/interp.h, InterpOps::leaf of csrc/leaf_vjp.h, the
INTERP instantiations of csrc/backward.hip and csrc/min_over_points.hip) at the forward's decision edges, against the
decision-conditioned float64 VJP in its trilinear mode (oracle/conditioned_vjp.py) -- nothing filtered out.  The sibling of
tests/test_autograd_edges_gpu.py, whose input generators, upstreams and bound it reuses.

Inputs: that file's edge points (range faces, surface-box faces, half-voxel planes, range edges and corners) plus the boundaries
only this mode has -- the lattice planes x_d = min_d + k res_d, k in {0, 1, two interior, n - 2, n - 1}, at the coordinate where
the forward's own s = (x - min) / res reaches k and one ulp to either side, on one, two and three axes at once -- over this file's
own 64 distinct trilinear leaves.  Every test first asserts the kernel's FORWARD (val, grad, leaf) equal to the CPU restatement
(tests/interp_ref.c) bit for bit on these inputs, then compares the backward.  All decisions of the reference (winner, range
test, cell, fractions, clamped axes) are the forward dtype's; only the differentiation is float64.

The bound is the sibling's, |got - want| <= c unit (n_chain + K) sum|term| with c = 4 and unit = 2^-24 / 2^-53, with K derived
for the trilinear terms.  Rounded operations along the longest path of one in-range term, from the records to the output
(a compiler's fma contraction only removes roundings):
    z-lerp e = fma(f, b - a, a): the subtraction, whose magnitude |a| + |b| is up to twice the blend's and so counts 2, and the
    fma: 3;  y-lerp: 3;  the difference y1 - y0 along the axis: 1  (the d f_y and d f_z paths are no longer: z-lerp 3, e1 - e0 1,
    1 - f_x 1, product 1, sum 1;  b - a 1, 1 - f_y 1, product 1, sum 1, 1 - f_x 1, product 1, sum 1)              7
    u_q = (L dgg)_q, a product and two sums: 3, and u_q * df: 1                                                      4
    the sum over the four channels (the first addition is to zero): 3;  the division by res: 1                      4
    dp = L^T dx, a product and two sums: 3   (dtf: dx_r p_j and its sum with gr_r dgg_j: 2; gr itself is three lerps, a
    product and a sum: 11)                                                                                           3
18 in all, more than the 16 the sibling's K = 8 covers twice over: K = 9, the smallest with c K >= 2 x 18.  The hinge's
upstream -(u (2 h)), h = margin - v, adds two roundings before the term: 20, K = 10 for hinge_over_points.  within_bound adds 8;
the tests pass n_chain + (K - 8).  K comes from this count, not from what the GPU returns.
n_chain is the sibling's: 0 for CachedSDF (one lane per point, no sum), A for dpoints of a composition (configurations in
registers, then the splits), nchunks + 14 for dtf (wave butterfly, LDS slots, slab rows)."""
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import conditioned_vjp as cv
from oracle import oracle
from tests import helpers as H
from tests import interp_ref as R
from tests.test_autograd_edges_gpu import (NPT, UNIT, assert_bound, edge_points, leaf_spec, loss_of, nchunks,
                                           object_points, transforms, ulps, upstreams)
from tests.test_interp_gpu import composed_ref_f32, composed_ref_f64

pytestmark = pytest.mark.gpu

K_TRI = 9     # see the module docstring
K_HINGE = 10


def extra(K):
    return K - 8  # within_bound's own "+ 8"


# ---------------------------------------------------------------- inputs
def grid_numbers_of(og, dtype):
    """(shape, min, res) of the oracle grid in the query dtype's statement"""
    c = og.c
    if dtype == np.float64:
        return np.array(c.shape[:], np.int32), np.array(c.dmin[:], np.float64), np.array(c.dres[:], np.float64)
    return np.array(c.shape[:], np.int32), np.array(c.fmin[:], np.float32), np.array(c.fres[:], np.float32)


def plane_coordinate(mn, res, k, dtype):
    """The smallest x of `dtype` whose forward quotient s = (x - mn) / res (the forward's two roundings) reaches k: where
    floor(s) steps to k -- s == k exactly whenever some x gives that."""
    x = dtype(np.float64(mn) + k * np.float64(res))
    s = lambda v: dtype(dtype(v - mn) / res)
    for _ in range(8):
        if not s(x) >= k:
            break
        x = np.nextafter(x, dtype(-np.inf))
    for _ in range(16):
        if s(x) >= k:
            break
        x = np.nextafter(x, dtype(np.inf))
    return x


def lattice_points(og, dtype, seed, rep=6, half_voxel=False):
    """Leaf-frame points of `dtype` on the lattice planes k in {0, 1, two interior, n - 2, n - 1} of every axis: at the
    coordinate where the forward's s reaches k and one ulp to either side, alone (the other coordinates random in range) and
    on two or three axes at once.  half_voxel: also points up to half a voxel beyond planes 0 and n - 1 (in range only under
    PVAMD_RULE_VALID_ON_INDEX)."""
    rng = np.random.default_rng(seed)
    shape, mn, res = grid_numbers_of(og, dtype)
    lo, hi = np.array(og.c.dmin[:]), np.array(og.c.dmax[:])
    planes = []
    for d in range(3):
        n = int(shape[d])
        inner = np.arange(2, max(n - 2, 3))  # the smallest leaves have a single interior plane
        ks = [0, 1] + sorted(rng.choice(inner, size=2, replace=len(inner) < 2).tolist()) + [n - 2, n - 1]
        planes.append([plane_coordinate(mn[d], res[d], k, dtype) for k in ks])

    def on_plane(d, count):
        base = np.array(planes[d], dtype)[rng.integers(0, 6, count)]
        step = rng.integers(-1, 2, count)
        out = base.copy()
        for u in (-1, 1):
            out = np.where(step == u, ulps(base, u, dtype), out)
        return out

    pts = []
    for d in range(3):
        for x in planes[d]:
            for u in (-1, 0, 1):
                p = rng.uniform(lo, hi, (rep, 3))
                p[:, d] = ulps(x, u, dtype)
                pts.append(p)
    for axes in ((0, 1), (0, 2), (1, 2), (0, 1, 2)):
        p = rng.uniform(lo, hi, (6 * rep, 3))
        for d in axes:
            p[:, d] = on_plane(d, len(p))
        pts.append(p)
    if half_voxel:
        for d in range(3):
            for below in (True, False):
                p = rng.uniform(lo, hi, (8 * rep, 3))
                t = rng.uniform(0.0, 0.5, len(p)) * np.float64(res[d])
                p[:, d] = lo[d] - t if below else lo[d] + (shape[d] - 1) * np.float64(res[d]) + t
                pts.append(p)
    return np.concatenate(pts).astype(dtype)


def cached_points(og, dtype, half_voxel=False):
    return np.concatenate((edge_points(og, dtype, seed=1), lattice_points(og, dtype, seed=2, half_voxel=half_voxel)))


def tri_object_points(ogs, m, A, dtype, seed, per_leaf=None, nudge=True):
    """object_points of the sibling (each leaf's edge points through one of its configurations) and, the same way, each leaf's
    lattice-plane points."""
    rng = np.random.default_rng(seed + 1000)
    edge = object_points(ogs, m, A, dtype, seed, per_leaf=None if per_leaf is None else per_leaf // 2, nudge=nudge)
    mm = m.double().numpy()
    out = [edge]
    for s, og in enumerate(ogs):
        x = lattice_points(og, NPT[dtype], seed + 500 + s, rep=1)
        if per_leaf is not None:
            x = x[rng.permutation(len(x))[:per_leaf - per_leaf // 2]]
        M = mm[s * A + (s % A)]
        p = ((x.astype(np.float64) - M[:3, 3]) @ M[:3, :3]).astype(NPT[dtype])
        if nudge:
            k = rng.integers(-2, 3, p.shape)
            for kk in (-2, -1, 1, 2):
                p = np.where(k == kk, ulps(p, kk, NPT[dtype]), p)
        out.append(p)
    return np.concatenate(out)


# ---------------------------------------------------------------- reference
def interp_of(leaves, dtype):
    return [R.grid_numbers(c, dtype == torch.float64) for c in leaves], R.cell


def ref_forward(leaves, ogs, m, A, pts, dtype, tri=True):
    """(val (A, P), grad (A, P, 3), leaf (A, P)) of the forward's CPU restatement"""
    if tri:
        fn = composed_ref_f64 if dtype == torch.float64 else composed_ref_f32
        return fn(leaves, m, torch.from_numpy(pts))
    fn = oracle.composed_query_f64 if dtype == torch.float64 else oracle.composed_query
    return fn(ogs, m.numpy(), A, pts)


def ref_vjp(leaves, ogs, m, A, pts, dv, dg, leaf, dtype, tri=True):
    return cv.composed_vjp(ogs, m.numpy(), A, pts, dv, dg, leaf=leaf, interp=interp_of(leaves, dtype) if tri else None)


def same_bits(got, want):
    return np.array_equal(got.detach().cpu().numpy().reshape(want.shape), want, equal_nan=True)


def check_tri(dp, dm, r, A, P, dtype, what, K=K_TRI):
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], dtype, A + extra(K), f"{what} dpoints")
    assert_bound(dm, r["dtf"], r["dtf_mag"], dtype, nchunks(P) + 14 + extra(K), f"{what} dtf")
    assert torch.equal(dm[:, 3], torch.zeros_like(dm[:, 3])), f"{what}: row 3 of dtf"


def run_tri(leaves, ogs, m, pts, batch, dtype, wv, wg, what, pshape=None):
    """forward (bit for bit against the restatement) and backward (within the bound) of one trilinear composition"""
    S = len(leaves)
    A = m.shape[0] // S
    P = pts.shape[0]
    comp = pv.ComposedSDF(leaves, None)
    mm = m.cuda().requires_grad_()
    comp.set_transforms(mm, batch_dim=batch)
    pt = torch.from_numpy(pts).reshape(pshape or (P, 3)).cuda().requires_grad_()
    val, grad = comp(pt)
    assert val.grad_fn is not None
    rv, rg, rl = ref_forward(leaves, ogs, m, A, pts, dtype)
    with torch.no_grad():
        leaf = comp._interp_forward(pt.detach(), want_leaf=True)[2]
    assert same_bits(val, rv) and same_bits(grad, rg) and same_bits(leaf, rl), f"{what}: forward"
    dp, dm = torch.autograd.grad(loss_of(val, grad, wv, wg), (pt, mm))
    dp = dp.reshape(-1, 3)
    r = ref_vjp(leaves, ogs, m, A, pts, wv, wg, rl, dtype)
    check_tri(dp, dm, r, A, P, dtype, what)
    return r, dp, dm


# ---------------------------------------------------------------- leaves
def build_tri_leaves(S, seed=0):
    leaves = []
    for s in range(S):
        sp = leaf_spec(s, seed)
        rng = H.padded_range(sp["gt"].bb.numpy(), sp["pad"], as_numpy=sp["f64"])
        leaves.append(pv.CachedSDF(f"tri{s}", sp["res"], rng, sp["gt"], device="cuda", cache_path=None, interpolation="trilinear"))
    return leaves


@pytest.fixture(scope="module")
def tri64():
    leaves = build_tri_leaves(64)
    return leaves, [H.oracle_grid_from_cached(c) for c in leaves]


def make_tri_cached(**kw):
    from tests.test_cached_gpu import make_cached
    c = make_cached(**kw)
    c.interpolation = "trilinear"  # this file's own instance
    return c


@pytest.fixture(scope="module")
def tri_caches():
    return {"f64": make_tri_cached(f64=True), "f32": make_tri_cached(f64=False),
            "f64_pad0": make_tri_cached(padding=0.0, f64=True), "f32_pad0": make_tri_cached(padding=0.0, f64=False)}


@pytest.fixture(scope="module")
def on_index_cache():
    from pytorch_volumetric_amd import voxel
    prev = voxel.INDEX_RULE
    voxel.INDEX_RULE = pv.RULE_VALID_ON_INDEX
    try:
        c = make_tri_cached(f64=True)
    finally:
        voxel.INDEX_RULE = prev
    assert c._view.rule == pv.RULE_VALID_ON_INDEX
    return c


# ---------------------------------------------------------------- cached
def run_cached(c, pts, dtype, upstream):
    """-> (dp, reference, (i, f, clamped) of every point by the forward's statements)"""
    f64 = dtype == torch.float64
    og = H.oracle_grid_from_cached(c)
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (P,), dtype, seed=2)
    p = torch.from_numpy(pts).cuda().requires_grad_()
    val, grad = c(p)
    num = R.grid_numbers(c, f64)
    nv, ng, oob = (oracle.cached_query_f64 if f64 else oracle.cached_query)(og, pts)
    rv, rg = R.forward(*num, pts, ~oob)
    assert same_bits(val, np.where(oob, nv, rv)) and same_bits(grad, np.where(oob[:, None], ng, rg)), "forward"
    (dp,) = torch.autograd.grad(loss_of(val, grad, wv, wg), p)
    r = cv.cached_vjp(og, pts, wv, wg, interp=([num], R.cell))
    assert np.array_equal(r["oob"].numpy(), oob)
    assert_bound(dp, r["dpoints"], r["dpoints_mag"], dtype, extra(K_TRI), "cached dpoints")
    return dp, r, R.cell(*num[1:], pts)


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["f64", "f32", "f64_pad0", "f32_pad0"])
def test_cached_backward_at_decision_edges(tri_caches, kind, dtype, upstream):
    c = tri_caches[kind]
    pts = cached_points(H.oracle_grid_from_cached(c), NPT[dtype])
    dp, r, (i, f, cl) = run_cached(c, pts, dtype, upstream)
    inr = ~r["oob"].numpy()
    top = np.array(c._view.shape) - 2
    assert int((~inr).sum()) > 100 and int(inr.sum()) > 100
    assert int((inr & ((f == 0) & ~cl).any(1)).sum()) > 50          # an integer s: the upper cell, f = 0
    assert int((inr & ((i == top) & (f == 1) & ~cl).any(1)).sum()) > 20  # s == n - 1: cell n - 2, f = 1, unclamped
    assert float(dp[torch.from_numpy(inr).cuda()].abs().sum()) > 0


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cached_backward_valid_on_index(on_index_cache, dtype, upstream):
    """PVAMD_RULE_VALID_ON_INDEX: half a voxel beyond the lattice is in range, s < 0 or s > n - 1 there, the axis clamped: no
    derivative along it."""
    c = on_index_cache
    pts = cached_points(H.oracle_grid_from_cached(c), NPT[dtype], half_voxel=True)
    dp, r, (i, f, cl) = run_cached(c, pts, dtype, upstream)
    inr = ~r["oob"].numpy()
    assert int((~inr).sum()) > 100 and int(inr.sum()) > 100
    hit = inr[:, None] & cl
    assert int(hit.any(1).sum()) > 50
    got = dp.cpu().numpy()
    assert np.array_equal(got[hit], np.zeros_like(got[hit]))
    assert np.array_equal(r["dpoints"].numpy()[hit], np.zeros(int(hit.sum())))


# ---------------------------------------------------------------- composed
@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tkind", ["exact", "random"])
def test_composed_8_distinct_leaves_with_a_tie(tri64, tkind, dtype, upstream):
    """S = 8 (leaf 7 is leaf 2 again, under the same transforms: an exact tie the first leaf must win), batch_dim = (2, 3),
    points shaped (2, N, 3)."""
    S, batch = 8, (2, 3)
    A = math.prod(batch)
    leaves = tri64[0][:7] + [tri64[0][2]]
    ogs = tri64[1][:7] + [tri64[1][2]]
    m = transforms(S, A, tkind, dtype, seed=3)
    m[7 * A:8 * A] = m[2 * A:3 * A]
    pts = tri_object_points(ogs[:7], m, A, dtype, seed=4, nudge=tkind == "random")
    pts = pts[:len(pts) // 2 * 2]
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (A, P), dtype, seed=5)
    r, dp, dm = run_tri(leaves, ogs, m, pts, batch, dtype, wv, wg, f"S=8 {tkind}", pshape=(2, P // 2, 3))
    won = set(r["leaf"].reshape(-1).tolist())
    assert 2 in won and 7 not in won and len(won) == 7
    assert torch.equal(dm[7 * A:8 * A], torch.zeros_like(dm[7 * A:8 * A]))  # the tie went to leaf 2
    assert int((~r["oob"]).sum()) > 100 and int(r["oob"].sum()) > 100


@pytest.mark.parametrize("upstream", ["val", "grad", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tkind", ["exact", "random"])
def test_composed_64_distinct_leaves_one_configuration(tri64, tkind, dtype, upstream):
    """S = 64 (present bit 63, LDS slot 63), tsf_batch None: one configuration, 150 points per leaf."""
    S, A = 64, 1
    leaves, ogs = tri64
    m = transforms(S, A, tkind, dtype, seed=6)
    pts = tri_object_points(ogs, m, A, dtype, seed=7, per_leaf=150, nudge=tkind == "random")
    P = pts.shape[0]
    wv, wg = upstreams(upstream, (P,), dtype, seed=8)
    r, _, _ = run_tri(leaves, ogs, m, pts, None, dtype, wv, wg, f"S=64 {tkind}")
    assert bool((r["leaf"] == 63).any()) and len(set(r["leaf"].reshape(-1).tolist())) == 64
    assert bool(((r["leaf"] == 63) & ~r["oob"]).any())


@pytest.mark.parametrize("P", [0, 1, 63, 65, 1023, 1025, 3089])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_partial_chunks(tri64, P, dtype):
    S, A = 8, 6
    leaves, ogs = tri64[0][8:16], tri64[1][8:16]
    m = transforms(S, A, "random", dtype, seed=9)
    rng = np.random.default_rng(11)
    pool = tri_object_points(ogs, m, A, dtype, seed=10)
    pool = np.concatenate((pool, rng.uniform(-0.55, 0.55, (max(0, P - len(pool)), 3)).astype(NPT[dtype])))
    pts = pool[rng.permutation(len(pool))[:P]]
    wv, wg = upstreams("both", (A, P), dtype, seed=12)
    if P == 0:
        comp = pv.ComposedSDF(leaves, None)
        mm = m.cuda().requires_grad_()
        comp.set_transforms(mm, batch_dim=(A,))
        pt = torch.from_numpy(pts).cuda().requires_grad_()
        val, grad = comp(pt)
        dp, dm = torch.autograd.grad(loss_of(val, grad, wv, wg), (pt, mm))
        assert dp.shape == (0, 3) and torch.equal(dm, torch.zeros_like(dm))
        return
    _, dp, dm = run_tri(leaves, ogs, m, pts, (A,), dtype, wv, wg, f"P={P}")
    assert dp.shape == (P, 3) and dm.shape == (S * A, 4, 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_64_leaves_8_splits(tri64, dtype):
    """S = 64, A = 8, P = 5000: five chunks (the last partial), eight splits of one configuration."""
    S, A, P = 64, 8, 5000
    leaves, ogs = tri64
    m = transforms(S, A, "random", dtype, seed=13)
    pool = tri_object_points(ogs, m, A, dtype, seed=14, per_leaf=100)
    pts = pool[np.random.default_rng(15).permutation(len(pool))[:P]]
    assert pts.shape[0] == P
    wv, wg = upstreams("both", (A, P), dtype, seed=16)
    r, _, _ = run_tri(leaves, ogs, m, pts, (A,), dtype, wv, wg, "S=64 A=8 P=5000")
    assert bool((r["leaf"] == 63).any())


# ---------------------------------------------------------------- impulses
IMP_S, IMP_A, IMP_P = 8, 6, 3089
SWEEP_P = [0, 63, 64, 1023, 1024, 3088]
SWEEP_A = [0, IMP_A - 1]


def wave_partner(p):
    return p + 1 if (p + 1) % 64 and p + 1 < IMP_P else p - 1


def interior_point(og, M, dtype):
    """An object-frame point that the matrix M takes strictly inside a cell next to the middle of og's lattice."""
    shape, mn, res = grid_numbers_of(og, np.float64)
    x = mn + (shape // 2 + np.array([0.37, 0.41, 0.29])) * res
    return ((x - M[:3, 3]) @ M[:3, :3]).astype(NPT[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_impulse_upstreams_hit_exactly_one_slot(tri64, dtype):
    """One (or two) non-zero pairs in range of their winners; every other dpoints row and dtf slot EXACTLY zero.  A value-only
    impulse reaches dpoints and dtf -- in the nearest mode an in-range value-only winner contributes nothing.
    The eight leaves are padded ones (their ranges contain their surface boxes: no pair is out of range with |d| = 0, where
    0 / 0 x 0 would reach dtf as it does in torch); the background points are farther than 0.28 from every lattice centre."""
    S, A, P = IMP_S, IMP_A, IMP_P
    pick = [s for s in range(64) if leaf_spec(s, 0)["pad"] == 0.03][:S]
    assert len(pick) == S
    leaves, ogs = [tri64[0][s] for s in pick], [tri64[1][s] for s in pick]
    m = transforms(S, A, "random", dtype, seed=21)
    mm64 = m.double().numpy()
    rng = np.random.default_rng(22)
    base = rng.uniform(-0.9, 0.9, (3 * P, 3))
    pts = base[np.abs(base).max(axis=1) > 0.66][:P].astype(NPT[dtype])
    assert pts.shape[0] == P
    winner, other = 1, 6
    for p in SWEEP_P:
        pts[p] = interior_point(ogs[winner], mm64[winner * A], dtype)
        pts[wave_partner(p)] = interior_point(ogs[other], mm64[other * A], dtype)
    comp = pv.ComposedSDF(leaves, None)
    mm = m.cuda().requires_grad_()
    comp.set_transforms(mm, batch_dim=(A,))
    pt = torch.from_numpy(pts).cuda().requires_grad_()
    val, grad = comp(pt)
    rv, rg, rl = ref_forward(leaves, ogs, m, A, pts, dtype)
    assert same_bits(val, rv) and same_bits(grad, rg), "forward"
    g = torch.Generator().manual_seed(23)
    for p in SWEEP_P:
        q = wave_partner(p)
        for a in SWEEP_A:
            for kind, pairs in (("val", [p]), ("both", [p]), ("both", [p, q])):
                dv = torch.zeros(A, P, dtype=dtype)
                dg = torch.zeros(A, P, 3, dtype=dtype) if kind == "both" else None
                for i in pairs:
                    dv[a, i] = torch.randn((), generator=g, dtype=torch.float64).to(dtype)
                    if dg is not None:
                        dg[a, i] = torch.randn(3, generator=g, dtype=torch.float64).to(dtype)
                dp, dm = torch.autograd.grad(loss_of(val, grad, dv, dg), (pt, mm), retain_graph=True)
                r = ref_vjp(leaves, ogs, m, A, pts[pairs], dv[:, pairs], None if dg is None else dg[:, pairs], rl[:, pairs], dtype)
                want_leaf = [winner, other][:len(pairs)]
                what = f"impulse p*={p} a*={a} {kind} pairs={pairs}"
                assert r["leaf"][a].tolist() == want_leaf and not bool(r["oob"][a].any()), what
                slots = [s * A + a for s in want_leaf]
                rest = torch.ones(S * A, dtype=torch.bool)
                rest[slots] = False
                assert torch.equal(dm[rest.cuda()], torch.zeros_like(dm[rest.cuda()])), what
                assert_bound(dm[slots], r["dtf"][slots], r["dtf_mag"][slots], dtype, extra(K_TRI), what + " dtf")
                assert bool((dm[slots, :3].abs().sum((1, 2)) > 0).all()), what
                rows = torch.zeros(P, dtype=torch.bool)
                rows[pairs] = True
                assert torch.equal(dp[~rows.cuda()], torch.zeros_like(dp[~rows.cuda()])), what
                assert_bound(dp[pairs], r["dpoints"], r["dpoints_mag"], dtype, extra(K_TRI), what + " dpoints")
                assert bool((dp[pairs].abs().sum(1) > 0).all()), what


# ---------------------------------------------------------------- fused reductions
def first_argmin(v):
    """first index of the minimum per row (no NaN among these values; -0.0 and +0.0 tie)"""
    assert not np.isnan(v).any()
    return np.argmin(v, axis=1)


def sub_composition(leaves, ogs, m, A, z):
    """the one-leaf composition of leaf z (None: all leaves)"""
    if z is None:
        return leaves, ogs, m
    return [leaves[z]], [ogs[z]], m[z * A:(z + 1) * A]


def accumulate(total, r, A, S, z):
    total["dpoints"] += r["dpoints"]
    total["dpoints_mag"] += r["dpoints_mag"]
    rows = slice(0, S * A) if z is None else slice(z * A, (z + 1) * A)
    total["dtf"][rows] += r["dtf"]
    total["dtf_mag"][rows] += r["dtf_mag"]


def empty_total(S, A, P):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    return dict(dpoints=z(P, 3), dpoints_mag=z(P, 3), dtf=z(S * A, 4, 4), dtf_mag=z(S * A, 4, 4))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tri", [False, True], ids=["nearest", "trilinear"])
def test_fused_reductions_against_the_conditioned_vjp(tri64, tri, dtype):
    """hinge_over_points (power 1 and 2) and min_over_points, overall and per leaf, over 8 distinct leaves at about 2k edge
    points: dpoints and dtf against the float64 VJP with the equivalent (A, P) upstream built here in float64 -- for the hinge
    -(u 2 h) or -u where margin - v >= 0 (v the restated forward's), for the minimum the reduction's upstream scattered at the
    restated forward's first argmin; per_leaf as the one-leaf compositions.  Not through __call__'s backward.
    n_chain, read off the kernels: hinge dpoints A (composed_backward_kernel: the configurations in registers, then the
    splits; reduce_splits_kernel) plus S - 1 < S for per_leaf (accumulate_kernel, leaf after leaf); hinge dtf nchunks + 14
    (wave butterfly, LDS slots, slab rows; per_leaf writes each leaf's rows in its own pass); minimum dpoints A Z
    (mop_scatter_kernel sums the pairs that selected a point, in pair order), minimum dtf 0 (mop_backward_kernel writes each
    row once)."""
    S, A = 8, 6
    # nearest leaves: the sibling's count (16, K = 8), plus the hinge's two roundings (18, K = 9)
    k_hinge, k_min = (K_HINGE, K_TRI) if tri else (9, 8)
    if tri:
        leaves, ogs = tri64[0][24:32], tri64[1][24:32]
    else:
        leaves = [pv.CachedSDF(f"near{s}", sp["res"], H.padded_range(sp["gt"].bb.numpy(), sp["pad"], as_numpy=sp["f64"]), sp["gt"],
                               device="cuda", cache_path=None) for s, sp in ((s, leaf_spec(s, 0)) for s in range(24, 32))]
        ogs = [H.oracle_grid_from_cached(c) for c in leaves]
    m = transforms(S, A, "random", dtype, seed=31)
    pts = tri_object_points(ogs, m, A, dtype, seed=32, per_leaf=250)
    P = pts.shape[0]
    comp = pv.ComposedSDF(leaves, None)
    mm = m.cuda().requires_grad_()
    comp.set_transforms(mm, batch_dim=(A,))
    pt = torch.from_numpy(pts).cuda().requires_grad_()
    # the restated forward, overall and per leaf; the kernels' forward is these bits
    fwd = {None: ref_forward(leaves, ogs, m, A, pts, dtype, tri)}
    for z in range(S):
        fwd[z] = ref_forward(*sub_composition(leaves, ogs, m, A, z), A, pts, dtype, tri)
    with torch.no_grad():
        val, grad = comp(pt.detach())
    assert same_bits(val, fwd[None][0]) and same_bits(grad, fwd[None][1]), "forward"
    g = torch.Generator().manual_seed(33)

    def vjp_of(z, dv, dg, sub=None, a=None):
        lv, og, mz = sub_composition(leaves, ogs, m, A, z)
        if sub is None:
            return ref_vjp(lv, og, mz, A, pts, dv, dg, fwd[z][2], dtype, tri)
        # one pair: configuration a alone, at the one point
        one = mz.reshape(len(lv), A, 4, 4)[:, a]
        return ref_vjp(lv, og, one, 1, pts[sub:sub + 1], dv, dg, fwd[z][2][a:a + 1, sub:sub + 1], dtype, tri)

    for per_leaf in (False, True):
        zs = list(range(S)) if per_leaf else [None]
        Z = len(zs)
        allv = np.stack([fwd[z][0] for z in zs], axis=1)  # (A, Z, P)
        margin = float(NPT[dtype](np.median(allv)))
        inside = int((margin - allv >= 0).sum())
        assert inside >= allv.size // 4 and allv.size - inside >= allv.size // 4
        # ---- hinge
        for power in (1, 2):
            what = f"hinge power={power} per_leaf={per_leaf}"
            u = torch.randn((A, Z), generator=g, dtype=torch.float64).to(dtype)
            out = comp.hinge_over_points(pt, margin, power=power, per_leaf=per_leaf)
            d = margin - allv.astype(np.float64)
            assert np.array_equal(out.counts.cpu().numpy().reshape(A, Z), (allv < margin).sum(-1)), what
            h = np.where(d > 0, d, 0.0).astype(NPT[dtype])  # each term rounded in the query dtype, summed in float64
            want = (h ** power).astype(NPT[dtype]).astype(np.float64).sum(-1)
            assert np.allclose(out.values.detach().cpu().numpy().reshape(A, Z), want, rtol=4 * UNIT[dtype], atol=0), what
            dp, dm = torch.autograd.grad((out.values.reshape(A, Z) * u.cuda()).sum(), (pt, mm))
            un = u.double().numpy()[:, :, None]
            dval = np.where(d >= 0, -(un * (2 * d)) if power == 2 else -un * np.ones_like(d), 0.0)
            total = empty_total(S, A, P)
            for k, z in enumerate(zs):
                accumulate(total, vjp_of(z, torch.from_numpy(dval[:, k]), None), A, S, z)
            assert_bound(dp, total["dpoints"], total["dpoints_mag"], dtype, A + (S if per_leaf else 0) + extra(k_hinge), what + " dpoints")
            assert_bound(dm, total["dtf"], total["dtf_mag"], dtype, nchunks(P) + 14 + extra(k_hinge), what + " dtf")
            assert torch.equal(dm[:, 3], torch.zeros_like(dm[:, 3])) and float(dp.abs().sum()) > 0 and float(dm.abs().sum()) > 0, what
        # ---- minimum
        what = f"min per_leaf={per_leaf}"
        uv = torch.randn((A, Z), generator=g, dtype=torch.float64).to(dtype)
        ug = torch.randn((A, Z, 3), generator=g, dtype=torch.float64).to(dtype)
        out = comp.min_over_points(pt, per_leaf=per_leaf)
        idx = np.stack([first_argmin(fwd[z][0]) for z in zs], axis=1)  # (A, Z)
        assert np.array_equal(out.indices.cpu().numpy().reshape(A, Z), idx), what
        rows = np.arange(A)
        assert same_bits(out.values, np.stack([fwd[z][0][rows, idx[:, k]] for k, z in enumerate(zs)], axis=1)), what
        assert same_bits(out.gradients, np.stack([fwd[z][1][rows, idx[:, k]] for k, z in enumerate(zs)], axis=1)), what
        dp, dm = torch.autograd.grad((out.values.reshape(A, Z) * uv.cuda()).sum() + (out.gradients.reshape(A, Z, 3) * ug.cuda()).sum(),
                                     (pt, mm))
        total = empty_total(S, A, P)
        for k, z in enumerate(zs):
            for a in range(A):
                i = int(idx[a, k])
                r = vjp_of(z, uv[a, k].reshape(1, 1), ug[a, k].reshape(1, 1, 3), sub=i, a=a)
                leaf = int(r["leaf"][0, 0]) if z is None else z
                total["dpoints"][i] += r["dpoints"][0]
                total["dpoints_mag"][i] += r["dpoints_mag"][0]
                total["dtf"][leaf * A + a] += r["dtf"][0 if z is not None else leaf]
                total["dtf_mag"][leaf * A + a] += r["dtf_mag"][0 if z is not None else leaf]
        assert_bound(dp, total["dpoints"], total["dpoints_mag"], dtype, A * Z + extra(k_min), what + " dpoints")
        assert_bound(dm, total["dtf"], total["dtf_mag"], dtype, extra(k_min), what + " dtf")
        hit = torch.zeros(P, dtype=torch.bool)
        hit[torch.from_numpy(idx.reshape(-1))] = True
        assert torch.equal(dp[~hit.cuda()], torch.zeros_like(dp[~hit.cuda()])), what
        assert torch.equal(dm[:, 3], torch.zeros_like(dm[:, 3])) and float(dm.abs().sum()) > 0, what
