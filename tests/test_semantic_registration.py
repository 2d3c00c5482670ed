"""CPU: the surface of pv.semantic_normal_equations and of refine_poses' semantics / targets / huber_delta (include/pvamd.h
"Semantic normal equations"), their argument checks, and the float64 restatement tests/semantic_registration_ref.py against
autograd and on the cases the feature exists for: free space that only pushes one way, and outliers.  No GPU: every check raises
or returns before a launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from pytorch_volumetric_amd import registration as reg
from tests import registration_ref as R
from tests import semantic_registration_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pvamd.h")).read()
NEW_SYMBOLS = ("pvamd_semantic_normal_eq_scratch_bytes", "pvamd_semantic_normal_eq")
U = 2.0 ** -53


def header_define(name):
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, re.M).group(1))


def test_exports_and_constants():
    assert pv.semantic_normal_equations is reg.semantic_normal_equations
    assert pv.SemanticNormalEquations is reg.SemanticNormalEquations
    assert pv.SemanticNormalEquations._fields == ("cost", "gradient", "hessian", "counts", "active", "outliers")
    assert pv.ChamferNormalEquations._fields == ("cost", "gradient", "hessian", "counts")  # unchanged
    want = {"SURFACE": 0, "FREE": 1, "OCCUPIED": 2, "IGNORE": 3}
    for name, value in want.items():
        assert header_define("PVAMD_POINT_" + name) == value == getattr(pv, "POINT_" + name) == getattr(_lib, "POINT_" + name)
        assert getattr(S, name) == value
    assert header_define("PVAMD_SEM_COUNTS") == 5 == _lib.SEM_COUNTS == S.COUNTS


def test_symbols_are_bound_and_declared_and_the_abi_number_stays():
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert "Semantic normal equations" in HEADER
    assert lib.pvamd_abi_version() == 16 == _lib.ABI_VERSION
    c = ctypes
    assert _lib.SIGNATURES["pvamd_semantic_normal_eq"] == (c.c_int, [
        c.POINTER(_lib.GridDesc), c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_double,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p])
    # the size is the exported function's: 28 sums and 5 counts of 8 bytes per pose and chunk, and no macro restates it
    assert "SEMANTIC_NORMAL_EQ_SCRATCH_BYTES" not in HEADER
    per = 8 * (_lib.REG_SUMS + _lib.SEM_COUNTS)
    assert _lib.semantic_normal_eq_scratch_bytes(1, 1) == per == lib.pvamd_semantic_normal_eq_scratch_bytes(1, _lib.REG_CHUNK)
    assert _lib.semantic_normal_eq_scratch_bytes(3, _lib.REG_CHUNK + 1) == per * 3 * 2
    assert lib.pvamd_semantic_normal_eq_scratch_bytes(0, 5) == 0 and lib.pvamd_semantic_normal_eq_scratch_bytes(5, 0) == 0


POSES = torch.eye(4).repeat(3, 1, 1)
CLOUD = torch.zeros(5, 3)
SPHERE = pv.SphereSDF(0.1)


@pytest.mark.parametrize("call", [pv.semantic_normal_equations, pv.refine_poses])
def test_input_errors_raise_before_a_launch(call):
    # what chamfer_normal_equations refuses
    for pts in (torch.zeros(5, 2), torch.zeros(2), torch.empty(0, 3)):
        with pytest.raises(ValueError):
            call(POSES, pts, SPHERE, huber_delta=0.01)
    with pytest.raises(TypeError):
        call(POSES, CLOUD, SPHERE, scale=True, huber_delta=0.01)
    # semantics
    for bad in (torch.zeros(5), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.bool), [0.0, 1.0, 2.0, 0.0, 0.0],
                [True, False, True, False, True]):
        with pytest.raises(TypeError):
            call(POSES, CLOUD, SPHERE, semantics=bad)
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros((5, 1), dtype=torch.int32), torch.zeros((), dtype=torch.uint8),
                [0, 1]):
        with pytest.raises(ValueError):
            call(POSES, CLOUD, SPHERE, semantics=bad)
    with pytest.raises(ValueError):  # the shape is that of points without its last dimension, not the flattened count
        call(POSES, torch.zeros(2, 3, 3), SPHERE, semantics=torch.zeros(6, dtype=torch.int64))
    # targets
    for bad in ("0.0", object(), torch.zeros(5, dtype=torch.complex64), torch.zeros(5, dtype=torch.bool), [1j] * 5):
        with pytest.raises(TypeError):
            call(POSES, CLOUD, SPHERE, targets=bad)
    for bad in (torch.zeros(4), torch.zeros(5, 1), 0.0, [0.0, 1.0]):
        with pytest.raises(ValueError):
            call(POSES, CLOUD, SPHERE, targets=bad)
    # huber_delta
    for bad in ("0.01", [0.01], torch.tensor(0.01), True, 1j):
        with pytest.raises(TypeError):
            call(POSES, CLOUD, SPHERE, huber_delta=bad)
    for bad in (0, 0.0, -0.0, -1e-3, -math.inf, math.nan):
        with pytest.raises(ValueError):
            call(POSES, CLOUD, SPHERE, huber_delta=bad)


def test_valid_arguments_pass_the_checks():
    """inf and an int for huber_delta, integer targets, every integer dtype of semantics, lists, leading dimensions."""
    pts = torch.zeros(2, 3, 3)
    assert reg._check_semantic_args(pts, None, None, None) == (None, None, None)
    assert reg._check_semantic_args(pts, None, None, math.inf)[2] == math.inf
    d = reg._check_semantic_args(pts, None, None, 1)[2]
    assert d == 1.0 and type(d) is float
    for dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        s, t, _ = reg._check_semantic_args(pts, torch.zeros((2, 3), dtype=dtype), torch.zeros((2, 3), dtype=torch.int32), None)
        assert s.dtype == dtype and t.dtype == torch.int32
    s, t, _ = reg._check_semantic_args(CLOUD, [0, 1, 2, 3, 300], [0.0, 0.1, 0.2, 0.3, 0.4], 0.5)
    assert torch.is_tensor(s) and torch.is_tensor(t) and s.tolist() == [0, 1, 2, 3, 300]


def _grid(finalized=1, oob=_lib.OOB_BOUNDING_BOX, vox=16):
    g = _lib.GridDesc()
    g.vox = vox  # never dereferenced: every call below returns before a launch
    for d in range(3):
        g.shape[d] = 4
    g.oob_mode, g.finalized = oob, finalized
    return g


def test_c_entry_point_checks_arguments_before_launching():
    lib = _lib.load()
    null = None
    g = ctypes.byref(_grid())
    ne = lib.pvamd_semantic_normal_eq
    inf = math.inf
    assert ne(g, 0, null, 2, null, 0, null, null, inf, null, null, null, null) == _lib.E_SHAPE   # N = 0
    assert ne(g, 0, null, -1, null, 5, null, null, inf, null, null, null, null) == _lib.E_SHAPE  # B < 0
    assert ne(g, 2, null, 2, null, 5, null, null, inf, null, null, null, null) == -4             # no such leaf mode
    assert ne(null, 0, null, 2, null, 5, null, null, inf, null, null, null, null) == -1          # no grid
    assert ne(ctypes.byref(_grid(oob=_lib.OOB_LOOKUP_GT_SDF)), 0, null, 2, null, 5, null, null, inf, null, null, null, null) == -4
    assert ne(ctypes.byref(_grid(finalized=0)), 0, null, 2, null, 5, null, null, inf, null, null, null, null) == -4
    for bad in (0.0, -0.0, -0.01, -inf, math.nan):
        assert ne(g, 0, null, 2, null, 5, null, null, bad, null, null, null, null) == -4, bad
        assert ne(g, 1, null, 0, null, 5, null, null, bad, null, null, null, null) == -4, bad    # before B = 0 returns
    assert ne(g, 1, null, 2, null, 5, null, null, 0.01, null, null, null, null) == -1            # W, points, outputs, scratch NULL
    assert ne(g, 1, null, 0, null, 5, null, null, inf, null, null, null, null) == 0              # B = 0: nothing to do
    assert ne(g, 0, null, 0, null, 5, null, null, 1e-300, null, null, null, null) == 0


def test_kinds_are_mapped_before_the_narrowing_cast():
    """Values that are not uint8 go through the Python mapping: -1, 4, 255 and 300 are IGNORE, not what the cast would make of
    them (300 -> 44, -1 -> 255 happens to be IGNORE too, 256 -> 0 would be SURFACE)."""
    cpu = torch.device("cpu")
    raw = torch.tensor([-1, 4, 255, 300, 256, 0, 1, 2, 3, -(2 ** 40), 2 ** 40 + 1])
    kinds, targets = reg._prepare_semantics(raw, None, cpu)
    assert targets is None and kinds.dtype == torch.uint8 and kinds.is_contiguous()
    assert kinds.tolist() == [3, 3, 3, 3, 3, 0, 1, 2, 3, 3, 3]
    assert reg._prepare_semantics(torch.tensor([-1, 2, -128], dtype=torch.int8), None, cpu)[0].tolist() == [3, 2, 3]
    assert reg._prepare_semantics(torch.tensor([255, 1, 4], dtype=torch.uint8), None, cpu)[0].tolist() == [3, 1, 3]
    kinds, targets = reg._prepare_semantics(torch.tensor([[0, 1], [2, 7]], dtype=torch.int32),
                                            torch.tensor([[1, 2], [3, 4]], dtype=torch.float64), cpu)
    assert kinds.tolist() == [0, 1, 2, 3] and targets.dtype == torch.float32 and targets.tolist() == [1.0, 2.0, 3.0, 4.0]
    assert reg._prepare_semantics(None, None, cpu) == (None, None)


# ---- the restatement ----
CENTRE = np.array([0.03, -0.02, 0.05])
RADIUS = 0.1


def _directions(n, rng):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _shell(n, lo, hi, seed, centre=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return np.asarray(centre) + _directions(n, rng) * rng.uniform(lo, hi, size=(n, 1))


def test_degenerate_restatement_is_the_chamfer_restatement():
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.2, 0.2, size=(300, 3)).astype(np.float32)
    v, n = R.sphere_vn(x, CENTRE, RADIUS)
    v, n = v.astype(np.float32), n.astype(np.float32)
    want = R.terms(v, n, x)
    for kinds, targets in ((None, None), (np.zeros(300, dtype=np.uint8), np.zeros(300, dtype=np.float32))):
        t, counts = S.sem_terms(v, n, x, kinds, targets, math.inf)
        assert np.array_equal(t, want)
        assert counts.tolist() == [300, 300, 0, 0, 0]


def test_restatement_gradient_against_autograd():
    """2 s1 = d / d xi of sum rho(r) at xi = 0 through x' = x + w cross x + u, by torch float64 autograd, for mixed kinds, non-zero
    targets and a delta that gives both branches.  No pair lies on a kink (r = 0 of a one-sided kind, |r| = delta): each is at
    least 1e-6 away, so the active set and the branch are constant around xi = 0.

    Bound per entry: (N + 16) 2^-53 sum_i m_i.  N - 1 roundings of either sum; per term at most 16 on the two sides together:
    the restatement's n = d / |d|, w = delta / a, q = w r, the cross product's two products and its difference, the product
    q j (7), autograd's norm and its backward (grad d / |d|: 3 with the norm's own), the cross product's backward (two products
    and a difference: 3), and slack for the accumulation into w's and u's gradient being a second sum.  m_i is |2 w r n_k| for
    a translation entry and 2 |w r| (|x_a n_b| + |x_b n_a|) for a rotation entry, the magnitudes of the cross product's two
    products: autograd forms x cross g from x = c + d, and what cancels against the closed form c cross n is relative to those
    products, not to their difference."""
    rng = np.random.default_rng(2)
    N, delta = 500, 0.02
    x = CENTRE + _directions(N, rng) * rng.uniform(0.02, 0.2, size=(N, 1))  # about as many points inside as outside
    kinds = rng.integers(0, 4, size=N)
    targets = rng.uniform(-0.01, 0.01, size=N).astype(np.float32)
    v, n = R.sphere_vn(x, CENTRE, RADIUS)
    r = S.residual(v, targets)
    assert (np.abs(r) > 1e-6).all() and (np.abs(np.abs(r) - delta) > 1e-6).all()
    t, counts = S.sem_terms(v, n, x, kinds, targets, delta)
    active = S.activity(r, kinds)[0]
    assert counts[1] > 50 and counts[2] > 20 and counts[3] > 20 and 20 < counts[4] < counts[1:4].sum() - 20
    for k in (S.FREE, S.OCCUPIED):  # each one-sided kind both active and inactive
        assert 0 < (active & (kinds == k)).sum() < (kinds == k).sum()
    assert not active[kinds == S.IGNORE].any()
    got = 2.0 * R.fsum_columns(t[:, 1:7])

    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    xt = torch.from_numpy(x)
    xp = xt + torch.linalg.cross(xi[3:].expand(N, 3), xt, dim=-1) + xi[:3]
    rt = (xp - torch.from_numpy(CENTRE)).norm(dim=-1) - RADIUS - torch.from_numpy(targets.astype(np.float64))
    rho = torch.where(rt.abs() > delta, delta * (2.0 * rt.abs() - delta), rt * rt)
    rho[torch.from_numpy(active)].sum().backward()
    want = xi.grad.numpy()

    w = np.where(np.abs(r) > delta, delta / np.abs(r), 1.0) * active
    g = 2.0 * np.abs(w * r)
    an, ax = np.abs(n), np.abs(x)
    mag = np.concatenate((g[:, None] * an, g[:, None] * np.stack((ax[:, 1] * an[:, 2] + ax[:, 2] * an[:, 1],
                                                                  ax[:, 2] * an[:, 0] + ax[:, 0] * an[:, 2],
                                                                  ax[:, 0] * an[:, 1] + ax[:, 1] * an[:, 0]), axis=-1)), axis=-1)
    bound = (N + 16) * U * R.fsum_columns(mag)
    err = np.abs(got - want)
    print("2 s1 vs autograd: worst error / bound =", (err / bound).max())
    assert (err <= bound).all(), (err, bound)
    # and the cost is sum rho
    assert abs(math.fsum(t[:, 0]) - float(rho.detach()[torch.from_numpy(active)].sum())) <= (N + 4) * U * math.fsum(np.abs(t[:, 0]))


def _one_sided_cloud():
    free = _shell(600, 0.1005, 0.13, seed=3)
    occupied = _shell(200, 0.05, 0.095, seed=4)
    pts = np.concatenate((free, occupied))
    kinds = np.concatenate((np.full(600, S.FREE), np.full(200, S.OCCUPIED)))
    return pts, kinds


def test_one_sided_points_on_their_own_side_add_exactly_nothing():
    """FREE points all outside the sphere and OCCUPIED points all inside: s0 = 0 and the 27 other sums exactly 0.0, and refine
    returns the input pose bit for bit with accepted == 1.  The sphere sits at the origin and the poses move a point by less than
    0.4 mm, so every point keeps its side (0.5 mm and 5 mm clear)."""
    pts, kinds = _one_sided_cloud()
    ev = S.sem_sphere_evaluator(pts, (0.0, 0.0, 0.0), RADIUS, kinds, None, 0.005)
    W0 = R.perturbed_poses(4, 0.0002, 0.001, seed=5)
    W0[0] = np.eye(4)
    sums = ev(W0)
    assert np.array_equal(sums, np.zeros_like(sums)) and not np.signbit(sums).any()
    assert np.array_equal(ev.counts, np.tile([800, 0, 0, 0, 0], (4, 1)))
    states, initial = R.refine(ev, W0, iterations=5)
    assert np.array_equal(initial, np.zeros(4))
    for b, st in enumerate(states):
        assert st.accepted == 1 and st.sums_acc[0] == 0.0
        assert np.array_equal(st.W_next().view(np.uint32), W0[b].view(np.uint32))
    # the same points with their kinds swapped are all active
    swapped = S.sem_sphere_evaluator(pts, (0.0, 0.0, 0.0), RADIUS, np.where(kinds == S.FREE, S.OCCUPIED, S.FREE), None, math.inf)
    assert (swapped(W0)[:, 0] > 0).all() and np.array_equal(swapped.counts, np.tile([800, 0, 200, 600, 0], (4, 1)))


def test_free_space_pulls_the_object_out_of_it():
    """The 600 FREE points of the shell, from a pose translated by 3 cm: some of them are inside the object at the start; 15
    iterations end at a strictly smaller cost with fewer of them inside."""
    pts = _shell(600, 0.1005, 0.13, seed=3)
    kinds = np.full(600, S.FREE)
    ev = S.sem_sphere_evaluator(pts, (0.0, 0.0, 0.0), RADIUS, kinds, None, math.inf)
    W0 = np.eye(4, dtype=np.float32)[None].copy()
    W0[0, 0, 3] = 0.03
    ev(W0)
    start = int(ev.counts[0, 2])
    states, initial = R.refine(ev, W0, iterations=15)
    final = states[0].sums_acc[0]
    ev(states[0].Wacc.astype(np.float32)[None])
    end = int(ev.counts[0, 2])
    print(f"free space: active {start} -> {end}, s0 {initial[0]:.6g} -> {final:.6g}, accepted {states[0].accepted}")
    assert start > 0 and initial[0] > 0
    assert final < initial[0]
    assert end < start
    assert (ev.counts[0, [1, 3, 4]] == 0).all()


def _centre_error(states, centre):
    return max(float(np.linalg.norm(st.Wacc[:, :3] @ centre + st.Wacc[:, 3] - centre)) for st in states)


def test_huber_weights_resist_outliers():
    """400 points on the sphere, the first 80 displaced by 5 cm along their normal and 4 cm along +y; four poses perturbed by up
    to 1 cm / 3 degrees, 20 iterations.  Least squares is pulled along +y by the displaced fifth; with delta = 5 mm their pull is
    bounded.  The centre error (the distance between the sphere's centre and its image under the refined pose) with Huber
    weights is below a fifth of the least-squares one."""
    rng = np.random.default_rng(6)
    n = _directions(400, rng)
    pts = CENTRE + RADIUS * n
    pts[:80] += 0.05 * n[:80] + np.array([0.0, 0.04, 0.0])
    W0 = R.perturbed_poses(4, 0.01, math.radians(3.0), seed=7)
    plain, _ = R.refine(S.sem_sphere_evaluator(pts, CENTRE, RADIUS), W0, iterations=20)
    huber_ev = S.sem_sphere_evaluator(pts, CENTRE, RADIUS, None, None, 0.005)
    huber, _ = R.refine(huber_ev, W0, iterations=20)
    e_plain, e_huber = _centre_error(plain, CENTRE), _centre_error(huber, CENTRE)
    print(f"centre error: least squares {1e3 * e_plain:.3f} mm, Huber (5 mm) {1e3 * e_huber:.3f} mm, ratio "
          f"{e_plain / e_huber:.1f}; outliers at the end {huber_ev.counts[:, 4].tolist()}")
    assert e_plain > 0.005  # the outliers do pull least squares
    assert e_huber < e_plain / 5.0, (e_huber, e_plain)


def test_edges_of_the_decisions():
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.2, 0.2, size=(12, 3)).astype(np.float32)
    n = _directions(12, rng).astype(np.float32)
    v = rng.uniform(-0.05, 0.05, size=12).astype(np.float32)
    # r == 0 exactly: FREE and OCCUPIED are inactive; SURFACE is active with a zero residual (its j j^T still enters)
    kinds = np.array([0, 1, 2] * 4)
    t, counts = S.sem_terms(v, n, x, kinds, v.copy(), 0.01)
    assert counts.tolist() == [12, 4, 0, 0, 0]
    assert np.array_equal(t[kinds != 0], np.zeros((8, 28)))
    assert np.array_equal(t[kinds == 0][:, :7], np.zeros((4, 7))) and (t[kinds == 0][:, 7] > 0).all()
    assert np.array_equal(t[kinds == 0][:, 7:], R.terms(v, n, x)[kinds == 0][:, 7:])
    # a == delta exactly is an inlier; one ulp below delta it is an outlier
    delta = float(abs(np.float64(v[5])))
    t, counts = S.sem_terms(v, n, x, None, None, delta)
    assert np.array_equal(t[5], R.terms(v, n, x)[5])
    below = np.nextafter(delta, 0.0)
    t2, counts2 = S.sem_terms(v, n, x, None, None, below)
    assert counts2[4] == counts[4] + 1 and t2[5, 0] == below * ((delta + delta) - below)
    # IGNORE and everything outside 0..3 add nothing, a NaN n and a NaN v included
    vn, nn = v.copy(), n.copy()
    nn[:6] = np.nan
    vn[3:6] = np.nan
    kinds = np.array([3, -1, 4, 255, 300, 3, 0, 1, 2, 0, 1, 2])
    t, counts = S.sem_terms(vn, nn, x, kinds, None, 0.01)
    assert np.array_equal(t[:6], np.zeros((6, 28))) and np.isfinite(t).all()
    ref, ref_counts = S.sem_terms(v[6:], n[6:], x[6:], kinds[6:], None, 0.01)
    assert np.array_equal(t[6:], ref) and counts[1:].tolist() == ref_counts[1:].tolist()
    # a NaN r of a one-sided kind fails both comparisons: active, and its sums are NaN
    t, counts = S.sem_terms(vn, n, x, np.array([0, 0, 0, 0, 1, 2] + [3] * 6), None, 0.01)
    assert counts[1:4].tolist() == [4, 1, 1] and np.isnan(t[3:6, 0]).all() and np.isfinite(t[:3]).all()
