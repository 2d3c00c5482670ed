"""CPU: the pose-refinement API surface (pv.chamfer_normal_equations, pv.refine_poses and their result tuples), the argument
checks, the _lib mirrors of the new C-ABI symbols (include/pvamd.h "Chamfer normal equations"), and the float64 restatement
tests/registration_ref.py against itself on an analytic sphere.  No GPU: every check raises or returns before a launch."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvamd_chamfer_normal_eq_scratch_bytes", "pvamd_chamfer_normal_eq", "pvamd_pose_lm_step")


def test_exports():
    assert pv.chamfer_normal_equations is reg.chamfer_normal_equations
    assert pv.refine_poses is reg.refine_poses
    assert pv.ChamferNormalEquations._fields == ("cost", "gradient", "hessian", "counts")
    assert pv.PoseRefinement._fields == ("world_to_object", "cost", "initial_cost", "accepted")
    assert (reg.LAMBDA_MIN, reg.LAMBDA_MAX) == (1e-12, 1e12) == (R.LAMBDA_MIN, R.LAMBDA_MAX)


def test_symbols_are_bound_and_declared_and_the_abi_number_stays():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pvamd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert "Chamfer normal equations" in open(os.path.join(ROOT, "include", "pvamd.h")).read()
    assert lib.pvamd_abi_version() == 16 == _lib.ABI_VERSION


def test_scratch_bytes_mirror():
    lib = _lib.load()
    assert (_lib.REG_CHUNK, _lib.REG_SUMS) == (2048, 28)
    assert _lib.chamfer_normal_eq_scratch_bytes(1, 1) == 232
    assert _lib.chamfer_normal_eq_scratch_bytes(1024, 16384) == 232 * 1024 * 8
    # these values come from the library: tests/test_abi.py compares the header's macro with the exported function
    assert _lib.chamfer_normal_eq_scratch_bytes(1, 2048) == 232 and _lib.chamfer_normal_eq_scratch_bytes(1, 2049) == 464
    assert lib.pvamd_chamfer_normal_eq_scratch_bytes(0, 5) == 0 and lib.pvamd_chamfer_normal_eq_scratch_bytes(5, 0) == 0


POSES = torch.eye(4).repeat(3, 1, 1)
CLOUD = torch.zeros(5, 3)
SPHERE = pv.SphereSDF(0.1)


@pytest.mark.parametrize("call", [pv.chamfer_normal_equations, pv.refine_poses])
def test_input_errors_raise_before_a_launch(call):
    for pts in (torch.zeros(5, 2), torch.zeros(5, 4), torch.zeros(2), torch.tensor(1.0)):
        with pytest.raises(ValueError):
            call(POSES, pts, SPHERE)
    for pts in (torch.empty(0, 3), torch.empty(2, 0, 3)):  # N = 0: the cost is a mean over the points
        with pytest.raises(ValueError):
            call(POSES, pts, SPHERE)
    for W in (torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 4, 3), torch.zeros(4, 5)):
        with pytest.raises(ValueError):
            call(W, CLOUD, SPHERE)
    for bad in ("1000", None, [1000.], torch.tensor(1000.), True, 1j):
        with pytest.raises(TypeError):
            call(POSES, CLOUD, SPHERE, scale=bad)
    for bad in (math.inf, math.nan):
        with pytest.raises(ValueError):
            call(POSES, CLOUD, SPHERE, scale=bad)
    with pytest.raises(TypeError):
        call(POSES, CLOUD, lambda x: (x[..., 0], x))


def test_refine_argument_errors_raise_before_a_launch():
    for bad in (0, -1):
        with pytest.raises(ValueError):
            pv.refine_poses(POSES, CLOUD, SPHERE, iterations=bad)
    for bad in (1.0, "10", None, True):
        with pytest.raises(TypeError):
            pv.refine_poses(POSES, CLOUD, SPHERE, iterations=bad)
    for bad in (0.0, -1e-3, math.inf, math.nan):
        with pytest.raises(ValueError):
            pv.refine_poses(POSES, CLOUD, SPHERE, damping=bad)
    for bad in (1.0, 0.5, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            pv.refine_poses(POSES, CLOUD, SPHERE, damping_up=bad)
    for bad in (0.0, -0.1, 1.5, math.inf, math.nan):
        with pytest.raises(ValueError):
            pv.refine_poses(POSES, CLOUD, SPHERE, damping_down=bad)
    for name in ("damping", "damping_up", "damping_down"):
        for bad in ("1", None, True, torch.tensor(0.5)):
            with pytest.raises(TypeError):
                pv.refine_poses(POSES, CLOUD, SPHERE, **{name: bad})


def _grid(finalized=1, oob=_lib.OOB_BOUNDING_BOX, vox=16):
    g = _lib.GridDesc()
    g.vox = vox  # never dereferenced: every call below returns before a launch
    for d in range(3):
        g.shape[d] = 4
    g.oob_mode, g.finalized = oob, finalized
    return g


def test_c_entry_points_check_arguments_before_launching():
    import ctypes
    lib = _lib.load()
    null = None
    g = ctypes.byref(_grid())
    ne = lib.pvamd_chamfer_normal_eq
    assert ne(g, 0, null, 2, null, 0, null, null, null, null) == _lib.E_SHAPE   # N = 0
    assert ne(g, 0, null, -1, null, 5, null, null, null, null) == _lib.E_SHAPE  # B < 0
    assert ne(g, 2, null, 2, null, 5, null, null, null, null) == -4             # no such leaf mode
    assert ne(null, 0, null, 2, null, 5, null, null, null, null) == -1          # no grid
    assert ne(ctypes.byref(_grid(oob=_lib.OOB_LOOKUP_GT_SDF)), 0, null, 2, null, 5, null, null, null, null) == -4
    assert ne(ctypes.byref(_grid(finalized=0)), 0, null, 2, null, 5, null, null, null, null) == -4
    assert ne(g, 1, null, 2, null, 5, null, null, null, null) == -1             # W, points, outputs, scratch NULL
    assert ne(g, 1, null, 0, null, 5, null, null, null, null) == 0              # B = 0: nothing to do
    step = lib.pvamd_pose_lm_step
    ok = (10.0, 0.1, 1e-12, 1e12)
    assert step(-1, null, 1, null, null, null, null, null, null, *ok, null) == _lib.E_SHAPE
    assert step(2, null, 1, null, null, null, null, null, null, *ok, null) == -1
    assert step(0, null, 1, null, null, null, null, null, null, *ok, null) == 0
    for bad in ((1.0, 0.1, 1e-12, 1e12), (10.0, 0.0, 1e-12, 1e12), (10.0, 1.5, 1e-12, 1e12), (10.0, 0.1, 0.0, 1e12),
                (10.0, 0.1, 1.0, 0.5), (10.0, 0.1, 1e-12, math.inf), (math.nan, 0.1, 1e-12, 1e12)):
        assert step(2, null, 1, null, null, null, null, null, null, *bad, null) == -4
    assert step(2, null, 2, null, null, null, null, null, null, *ok, null) == -4  # first is 0 or 1


# ---- the restatement against itself, on an analytic float64 sphere whose residual is exactly differentiable ----
def _sphere_cloud(n, centre, radius, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return np.asarray(centre) + radius * d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_reference_gradient_is_half_the_central_difference_of_its_cost():
    """cost(xi) at the pose Exp(xi) W, h = 1e-4: the central difference errs by O(h^2) + O(eps / h), so 1e-6 of |gradient|_inf."""
    centre, radius = np.array([0.03, -0.02, 0.05]), 0.1
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.15, 0.15, size=(400, 3)) + centre  # off the surface: non-zero residuals
    W = R.perturbed_poses(1, 0.02, 0.1, seed=2)[0, :3].astype(np.float64)

    def cost_at(Wm):
        x = pts @ Wm[:, :3].T + Wm[:, 3]
        v, n = R.sphere_vn(x, centre, radius)
        return R.unpack(R.raw_sums(v, n, x), len(pts), 1.)

    _, grad, hess = cost_at(W)
    assert np.array_equal(hess, hess.T)
    h = 1e-4
    fd = np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        fd[k] = (cost_at(R.retract(W, e))[0] - cost_at(R.retract(W, -e))[0]) / (2 * h)
    assert np.abs(grad - 0.5 * fd).max() <= 1e-6 * np.abs(grad).max(), (grad, 0.5 * fd)


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (0.03, -0.02, 0.05)])
def test_reference_loop_converges_on_a_zero_residual_sphere(centre):
    """16 poses perturbed by <= 2 cm / 5 degrees, 500 points on the sphere's surface (r = 0.1), the default damping schedule, 10
    evaluations after the first: the unscaled cost s0 / N falls to <= 1e-20.  The Hessian has rank 3 (a sphere fixes no
    rotation about its centre): the centred sphere exercises D_k = 1 on a zero diagonal, the off-centre one Marquardt damping
    on a singular S2.

    The 1e-20 bar is asked of the loop's own float64 arithmetic (rounded=False: float64 start poses, each trial pose evaluated
    as the step produced it).  With float32 poses, as the kernels read them, no evaluation count reaches 1e-20 (observed here:
    1e-18 to 8e-18 after 10 and after 30 evaluations): the start pose and every trial pose have each entry off by up to 2^-25
    of itself, and a left-multiplied twist cannot undo a rounded rotation block.  A point then moves by up to e = 2 * 2^-25
    (|R row|_1 |p|_inf + |t|_inf) <= 2^-24 (sqrt(3) |p|_inf + |t|_inf) per component, and the residual of a surface point is
    at most |e|_2 <= sqrt(3) e: the float32 loop is asserted against that floor squared.

    The evaluator hands over the sphere's closed-form Jacobian (x cross n = c cross n: exactly zero for the centred sphere, the
    case D_k = 1 is for).  A finding, not a bar: with x cross n formed numerically from a rounded n, the centred sphere's
    rotational diagonal is rounding noise (about N (u |x|)^2) instead of zero, damping relative to it tames nothing, and the
    same loop stalls at 6.9e-5 after 10 evaluations and 4.9e-8 after 40: the rule recognises an exactly unobserved axis only."""
    radius, n = 0.1, 500
    pts = _sphere_cloud(n, centre, radius, seed=3)
    W0 = R.perturbed_poses(16, 0.02, math.radians(5.0), seed=4, dtype=np.float64)
    states, initial = R.refine(R.sphere_evaluator(pts, centre, radius), W0, iterations=10, rounded=False)
    cost = np.array([s.sums_acc[0] for s in states]) / n
    assert (initial / n > 1e-6).all()  # the start is really perturbed
    print("float64 trial poses: max cost", cost.max())
    assert (cost <= 1e-20).all(), cost
    assert all(s.accepted >= 2 for s in states)
    states, _ = R.refine(R.sphere_evaluator(pts, centre, radius), W0.astype(np.float32), iterations=10)
    cost = np.array([s.sums_acc[0] for s in states]) / n
    floor = math.sqrt(3.0) * 2.0 ** -24 * (math.sqrt(3.0) * np.abs(pts).max() + max(abs(s.Wacc[:, 3]).max() for s in states))
    print("float32 trial poses: max cost", cost.max(), "floor", floor ** 2)
    assert (cost <= floor ** 2).all(), (cost, floor ** 2)


def test_reference_step_decisions():
    """accept / reject / NaN / clamps / zero step of the restatement's own step (the GPU test compares the kernel with these)."""
    rng = np.random.default_rng(5)
    M = rng.normal(size=(6, 6))
    S2 = M @ M.T + 6 * np.eye(6)
    sums = np.concatenate(([2.0], rng.normal(size=6), [S2[r, c] for r, c in R.TRIU]))
    st = R.LMState(Wtry=np.eye(4)[:3].copy(), lam=1e-3)
    R.lm_step(st, sums, True)
    assert st.accepted == 1 and st.lam == 1e-3 * 0.1
    A = R.damped_matrix(sums, st.lam)
    assert np.allclose(A @ st.xi, -sums[1:7], rtol=1e-10, atol=1e-12)
    worse = sums.copy()
    worse[0] = 3.0
    lam = st.lam
    R.lm_step(st, worse, False)
    assert st.accepted == 1 and st.lam == lam * 10.0 and st.sums_acc[0] == 2.0
    nan = sums.copy()
    nan[0] = math.nan
    R.lm_step(st, nan, False)
    assert st.accepted == 1 and st.sums_acc[0] == 2.0
    st.lam = 1e12
    R.lm_step(st, worse, False)
    assert st.lam == 1e12
    st.lam = 1e-12
    better = sums.copy()
    better[0] = 1.0
    R.lm_step(st, better, False)
    assert st.lam == 1e-12 and st.accepted == 2
    zero = better.copy()
    zero[0], zero[1:7] = 0.5, 0.0
    R.lm_step(st, zero, False)
    assert np.all(st.xi == 0.0) and np.array_equal(st.Wtry, st.Wacc)
