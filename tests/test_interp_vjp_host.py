"""CPU: the trilinear mode of the decision-conditioned float64 VJP (oracle/conditioned_vjp.py with `interp`) and the cell entry
points of tests/interp_ref.c, on grids filled from an analytic field (no CachedSDF, no GPU).

The reference of tests/test_interp_edges_gpu.py is checked here against difference quotients of the forward's own restatement:
central ones away from cell faces, the right-sided one at an integer s (the upper cell), the left-sided one at s == n - 1
(cell n - 2 with f = 1), an exact zero on a clamped axis; and the float32 cell decisions are shown to be the forward's (cell +
blend is interp_forward_f32 bit for bit) and NOT what float64 arithmetic on the same points would decide."""
import numpy as np
import pytest
import torch

from oracle import conditioned_vjp as cv
from oracle import oracle
from tests import interp_ref as R


def field(x):
    """A smooth, non-multilinear field and three more channels: (n, 4) float64."""
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    return np.stack((np.sin(3 * a) * np.cos(2 * b) + c * c, np.cos(a + 2 * c) * b, a * b * c + np.sin(b), np.exp(0.5 * a) - b * c), -1)


def make_grid(mn, res, shape, rule=0):
    """(oracle grid, records [n][4] float32) of `field` sampled at mn + idx res; a float64 range (index_f64)."""
    mn, res, shape = np.asarray(mn, np.float64), np.asarray(res, np.float64), np.asarray(shape, np.int32)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    rec = np.ascontiguousarray(field(mn + idx * res).astype(np.float32))
    mx = mn + (shape - 1) * res
    bb = np.stack((mn + 0.2 * (mx - mn), mx - 0.2 * (mx - mn)), axis=1)
    og = oracle.Grid(rec[:, 0].reshape(shape), rec[:, 1:], mn, mx, bb, index_f64=True, rule=rule)
    return og, rec


def numbers(og, rec, f64):
    c = og.c
    if f64:
        return rec, np.array(c.shape[:], np.int32), np.array(c.dmin[:], np.float64), np.array(c.dres[:], np.float64)
    return rec, np.array(c.shape[:], np.int32), np.array(c.fmin[:], np.float32), np.array(c.fres[:], np.float32)


def upstream(P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, generator=g, dtype=torch.float64), torch.randn(P, 3, generator=g, dtype=torch.float64)


def loss_f64(num, pts, wv, wg):
    """sum_p wv val + wg . grad of the float64 forward restatement, per point (P,)"""
    val, grad = R.forward(*num, pts, np.ones(len(pts), bool))
    return val * wv.numpy() + (grad * wg.numpy()).sum(-1)


def quotient(num, pts, wv, wg, d, h, side):
    """difference quotient along axis d: side 0 central, +1 right-sided, -1 left-sided"""
    e = np.zeros(3)
    e[d] = h
    if side == 0:
        return (loss_f64(num, pts + e, wv, wg) - loss_f64(num, pts - e, wv, wg)) / (2 * h)
    if side > 0:
        return (loss_f64(num, pts + e, wv, wg) - loss_f64(num, pts, wv, wg)) / h
    return (loss_f64(num, pts, wv, wg) - loss_f64(num, pts - e, wv, wg)) / h


# dyadic lattice: mn + k res is exact in float64, so "an integer s" is one
MN, RES, SHAPE = np.array([-0.5, 0.25, -1.0]), np.array([0.125, 0.0625, 0.25]), np.array([7, 9, 6])
H = 2.0 ** -20  # along one axis the interpolant is linear within a cell: a quotient is exact up to rounding (~2^-53 / H)
QTOL = 1e-8


def vjp_f64(og, rec, pts, wv, wg):
    r = cv.cached_vjp(og, pts, wv, wg, interp=([numbers(og, rec, True)], R.cell))
    assert not bool(r["oob"].any())
    return r


def test_vjp_equals_central_differences_away_from_edges():
    og, rec = make_grid(MN, RES, SHAPE)
    rng = np.random.default_rng(0)
    s = rng.integers(0, SHAPE - 1, (400, 3)) + rng.uniform(0.01, 0.99, (400, 3))
    pts = MN + s * RES
    wv, wg = upstream(len(pts), 1)
    r = vjp_f64(og, rec, pts, wv, wg)
    num = numbers(og, rec, True)
    for d in range(3):
        want = quotient(num, pts, wv, wg, d, H, 0)
        assert np.allclose(r["dpoints"][:, d].numpy(), want, rtol=QTOL, atol=QTOL)
    assert float(r["dpoints"].abs().min()) > 0
    # the magnitudes dominate the values (every difference b - a as |a| + |b|)
    assert bool((r["dpoints_mag"] >= r["dpoints"].abs() * (1 - 1e-12)).all())

    def f(p):  # torch.autograd.gradcheck's own differences agree as well
        class Fwd(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q):
                ctx.save_for_backward(q)
                v, g = R.forward(*num, q.detach().numpy(), np.ones(len(q), bool))
                return torch.from_numpy(v), torch.from_numpy(g)

            @staticmethod
            def backward(ctx, dv, dg):
                (q,) = ctx.saved_tensors
                with torch.enable_grad():  # the reference differentiates with autograd itself
                    return cv.cached_vjp(og, q.detach().numpy(), dv, dg, interp=([num], R.cell))["dpoints"]
        return Fwd.apply(p)

    x = torch.from_numpy(pts[:20].copy()).requires_grad_()
    assert torch.autograd.gradcheck(f, (x,), eps=H, atol=1e-7, rtol=1e-7)


@pytest.mark.parametrize("where", ["integer", "top"])
def test_one_sided_derivative_on_lattice_planes(where):
    """At an integer s the cell is the upper one (f = 0): the right-sided quotient.  At s == n - 1 it is cell n - 2 with f = 1,
    unclamped: the left-sided quotient.  Neither is the mean of the two sides."""
    og, rec = make_grid(MN, RES, SHAPE)
    rng = np.random.default_rng(2)
    n = 300
    s = rng.integers(0, SHAPE - 1, (n, 3)) + rng.uniform(0.01, 0.99, (n, 3))
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)
    s[rows, axis] = (SHAPE[axis] - 1) if where == "top" else rng.integers(1, SHAPE[axis] - 1)
    pts = MN + s * RES
    wv, wg = upstream(n, 3)
    r = vjp_f64(og, rec, pts, wv, wg)
    num = numbers(og, rec, True)
    i, f, cl = R.cell(*num[1:], pts)
    assert not cl.any()
    if where == "top":
        assert np.array_equal(i[rows, axis], SHAPE[axis] - 2) and np.array_equal(f[rows, axis], np.ones(n))
    else:
        assert np.array_equal(i[rows, axis], s[rows, axis].astype(np.int64)) and np.array_equal(f[rows, axis], np.zeros(n))
    side = -1 if where == "top" else 1
    got = r["dpoints"].numpy()[rows, axis]
    want = np.stack([quotient(num, pts, wv, wg, d, H, side) for d in range(3)], -1)[rows, axis]
    assert np.allclose(got, want, rtol=QTOL, atol=QTOL)
    if where == "integer":  # and it differs from the other side's slope: the lattice plane is a kink
        other = np.stack([quotient(num, pts, wv, wg, d, H, -side) for d in range(3)], -1)[rows, axis]
        assert (np.abs(got - other) > 1e-3 * np.abs(got)).mean() > 0.9


def test_clamped_axis_is_exactly_zero():
    """Under PVAMD_RULE_VALID_ON_INDEX half a voxel beyond the lattice is in range: s < 0 or s > n - 1, c != s, no derivative
    along that axis -- and the full derivative along the others."""
    og, rec = make_grid(MN, RES, SHAPE, rule=1)
    rng = np.random.default_rng(4)
    n = 300
    s = rng.integers(0, SHAPE - 1, (n, 3)) + rng.uniform(0.01, 0.99, (n, 3))
    axis = rng.integers(0, 3, n)
    rows = np.arange(n)
    below = rng.random(n) < 0.5
    s[rows, axis] = np.where(below, -rng.uniform(0.01, 0.49, n), SHAPE[axis] - 1 + rng.uniform(0.01, 0.49, n))
    pts = MN + s * RES
    wv, wg = upstream(n, 5)
    r = vjp_f64(og, rec, pts, wv, wg)
    dp, mag = r["dpoints"].numpy(), r["dpoints_mag"].numpy()
    assert np.array_equal(dp[rows, axis], np.zeros(n)) and np.array_equal(mag[rows, axis], np.zeros(n))
    num = numbers(og, rec, True)
    free = np.ones((n, 3), bool)
    free[rows, axis] = False
    want = np.stack([quotient(num, pts, wv, wg, d, H, 0) for d in range(3)], -1)
    assert np.allclose(dp[free], want[free], rtol=QTOL, atol=QTOL) and np.abs(dp[free]).min() > 0
    # the forward is constant along the clamped axis there: the quotient is zero too
    assert np.array_equal(want[rows, axis], np.zeros(n))


def test_float32_cells_are_the_forwards_and_not_the_float64_ones():
    """Lattice planes of a non-dyadic grid, exactly (as float32 rounds them) and at +-1 ulp: the float32 cell decisions feed the
    blend to interp_forward_f32's bits, and some of them differ from what float64 arithmetic on the same float32 numbers
    decides -- so a reference that re-derived them in float64 would differentiate another cell at these points."""
    mn, res, shape = np.array([-0.117, 0.033, -0.201]), np.array([0.01, 0.0125, 0.02]), np.array([24, 17, 13])
    og, rec = make_grid(mn, res, shape)
    num32 = numbers(og, rec, False)
    fmn, fres = num32[2], num32[3]
    rng = np.random.default_rng(6)
    pts = []
    for d in range(3):
        for k in range(shape[d]):
            for u in (-1, 0, 1):
                p = (fmn.astype(np.float64) + rng.uniform(0.05, shape - 1.05, (4, 3)) * fres).astype(np.float32)
                plane = np.float32(np.float32(fmn[d]) + np.float32(k) * np.float32(fres[d]))
                if u:
                    plane = np.nextafter(plane, np.float32(np.inf if u > 0 else -np.inf))
                p[:, d] = plane
                pts.append(p)
    pts = np.concatenate(pts)
    i32, f32, c32 = R.cell(*num32[1:], pts)
    assert f32.dtype == np.float32
    val, grad = R.forward(*num32, pts, np.ones(len(pts), bool))
    bv, bg = R.blend(rec, shape, i32, f32)
    assert np.array_equal(bv, val) and np.array_equal(bg, grad)
    i64, f64, c64 = R.cell(shape, fmn.astype(np.float64), fres.astype(np.float64), pts.astype(np.float64))
    differ = (i32 != i64).any(1) | (c32 != c64).any(1)
    assert int(differ.sum()) >= 1, "the edge inputs are not edges"
    assert int(((f32 == 0).any(1) & ~c32.any(1)).sum()) > 20  # integer s reached in float32
    # the float32-conditioned VJP at those points is the derivative of the float32 forward's own cell: blending the float32
    # cell's records in float64 and differencing in f reproduces it
    wv, wg = upstream(len(pts), 7)
    valid = ~oracle.cached_query(og, pts)[2]
    r = cv.cached_vjp(og, pts, wv, wg, interp=([num32], R.cell))
    assert np.array_equal(~r["oob"].numpy(), valid) and int((valid & differ).sum()) >= 1
    h = 2.0 ** -12
    for d in range(3):
        fp, fm = f32.astype(np.float64), f32.astype(np.float64)
        fp[:, d] += h
        fm[:, d] -= h
        lp = [R.blend(rec, shape, i32, f) for f in (fp, fm)]
        q = ((lp[0][0] - lp[1][0]) * wv.numpy() + ((lp[0][1] - lp[1][1]) * wg.numpy()).sum(-1)) / (2 * h) / np.float64(fres[d])
        q = np.where(c32[:, d], 0.0, q)
        assert np.allclose(r["dpoints"].numpy()[valid, d], q[valid], rtol=1e-9, atol=1e-9)
