"""Float64 numpy restatement of include/pvamd.h "Chamfer normal equations": the per-pair terms and their sums, the
Levenberg-Marquardt step of pvamd_pose_lm_step and the loop of refine_poses.  Test infrastructure: the product never imports it.
The arithmetic is plain float64 (no fused multiply-add), so it agrees with the kernels to rounding, not bit for bit; the decisions
(accept / reject, the damping, the failed-pivot rule, the zero step) are the same statements."""
import math
from dataclasses import dataclass, field

import numpy as np

SUMS = 28
LAMBDA_MIN = 1e-12
LAMBDA_MAX = 1e12
TRIU = [(r, c) for r in range(6) for c in range(r, 6)]


def jacobian(x, n):
    """j = (n, x cross n) in float64 from (N, 3) x and n (float32 inputs: every product is exact, every component rounds once)."""
    x = np.asarray(x).astype(np.float64)
    n = np.asarray(n).astype(np.float64)
    return np.concatenate((n, np.cross(x, n)), axis=-1)


def terms(v, n, x, j=None):
    """(N, 28) float64 terms of one pose: v v, v j (6), j_r j_c for r <= c (21); each product rounded once.  j: the (N, 6)
    Jacobian rows when the caller has them in closed form, else jacobian(x, n)."""
    v = np.asarray(v).astype(np.float64).reshape(-1)
    j = (jacobian(x, n) if j is None else np.asarray(j, dtype=np.float64)).reshape(-1, 6)
    cols = [v * v] + [v * j[:, k] for k in range(6)] + [j[:, r] * j[:, c] for r, c in TRIU]
    return np.stack(cols, axis=-1)


def raw_sums(v, n, x, j=None):
    return terms(v, n, x, j).sum(axis=0)


def fsum_columns(t):
    """Exactly rounded column sums of an (N, K) array."""
    return np.array([math.fsum(t[:, k]) for k in range(t.shape[1])])


def unpack(sums, N, scale=1000.):
    """cost, gradient (6,), hessian (6, 6) from the 28 raw sums."""
    k = scale * scale / N
    H = np.zeros((6, 6))
    for e, (r, c) in enumerate(TRIU):
        H[r, c] = H[c, r] = sums[7 + e]
    return sums[0] * k, sums[1:7] * k, H * k


def damped_matrix(sums, lam):
    """A = S2 + lam D of step b, D_k = S2_kk where positive and 1 elsewhere."""
    A = unpack(sums, 1, 1.)[2].copy()
    for k in range(6):
        d = A[k, k] if A[k, k] > 0.0 else 1.0
        A[k, k] = A[k, k] + lam * d
    return A


def cholesky_solve(A, rhs):
    """(xi, ok): Cholesky without pivoting in the kernel's order; ok is False for a pivot that is not positive and finite or a
    non-finite solution."""
    L = np.zeros((6, 6))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (d > 0.0) or not (d < math.inf):
                ok = False
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        xi = np.zeros(6)
        for i in range(6):
            s = rhs[i]
            for k in range(i):
                s = s - L[i, k] * xi[k]
            xi[i] = s / L[i, i]
        for i in range(5, -1, -1):
            s = xi[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * xi[k]
            xi[i] = s / L[i, i]
    ok = ok and bool(np.all(np.isfinite(xi)))
    return xi, ok


def exp_so3(w):
    """Rodrigues: I + a K + c K^2, a = sin th / th, c = (sin(th / 2) / (th / 2))^2 / 2; the series below th < 1e-8."""
    wx, wy, wz = (float(t) for t in w)
    th2 = wx * wx + wy * wy + wz * wz
    th = math.sqrt(th2)
    if th < 1e-8:
        a, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a = math.sin(th) / th
        q = math.sin(0.5 * th) / (0.5 * th)
        c = 0.5 * q * q
    K = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    E = c * np.outer(w, w) + a * K
    E[0, 0] = 1.0 - c * (wy * wy + wz * wz)
    E[1, 1] = 1.0 - c * (wx * wx + wz * wz)
    E[2, 2] = 1.0 - c * (wx * wx + wy * wy)
    return E


def retract(W, xi):
    """[Exp(w) R, Exp(w) t + u] from W = [R, t] (3, 4); a zero step returns W itself."""
    xi = np.asarray(xi, dtype=np.float64)
    if np.all(xi == 0.0):
        return W.copy()
    out = exp_so3(xi[3:]) @ W
    out[:, 3] += xi[:3]
    return out


@dataclass
class LMState:
    """One pose of pvamd_pose_lm_step's state."""
    Wtry: np.ndarray
    lam: float
    Wacc: np.ndarray = None
    sums_acc: np.ndarray = field(default_factory=lambda: np.full(SUMS, np.nan))
    accepted: int = 0
    xi: np.ndarray = None  # the last step (not part of the kernel's state; kept for the tests)

    def W_next(self):
        out = np.zeros((4, 4), dtype=np.float32)
        out[:3] = self.Wtry.astype(np.float32)
        out[3, 3] = 1.0
        return out


def lm_step(st, sums, first, up=10., down=0.1, lambda_min=LAMBDA_MIN, lambda_max=LAMBDA_MAX):
    """pvamd_pose_lm_step for one pose, in place."""
    sums = np.asarray(sums, dtype=np.float64)
    if first or sums[0] < st.sums_acc[0]:
        st.Wacc = st.Wtry.copy()
        st.sums_acc = sums.copy()
        st.lam = max(st.lam * down, lambda_min)
        st.accepted += 1
    else:
        st.lam = min(st.lam * up, lambda_max)
    xi, ok = cholesky_solve(damped_matrix(st.sums_acc, st.lam), -st.sums_acc[1:7])
    if not ok:
        xi = np.zeros(6)
        st.lam = min(st.lam * up, lambda_max)
    st.xi = xi
    st.Wtry = retract(st.Wacc, xi)
    return st


def refine(evaluate, W0, iterations=10, damping=1e-3, up=10., down=0.1, rounded=True):
    """refine_poses' loop.  evaluate((B, 4, 4) float32) -> (B, 28) raw sums.  W0: (B, 4, 4) float32.  Returns the states and the
    initial s0.  rounded=False keeps W0 in float64 and hands evaluate the float64 trial poses instead of their float32 rounding
    (what the kernels read): the loop's own arithmetic, without the cost floor that a float32 pose (rounded, so not exactly
    rigid) puts under a zero-residual problem."""
    W0 = np.asarray(W0, dtype=np.float32 if rounded else np.float64)
    states = [LMState(Wtry=W0[b, :3].astype(np.float64), lam=damping) for b in range(len(W0))]
    initial = None
    for it in range(iterations + 1):
        poses = np.stack([s.W_next() if rounded else np.vstack((s.Wtry, [[0.0, 0.0, 0.0, 1.0]])) for s in states])
        sums = np.asarray(evaluate(poses), dtype=np.float64)
        if it == 0:
            initial = sums[:, 0].copy()
        for b, st in enumerate(states):
            lm_step(st, sums[b], it == 0, up, down)
    return states, initial


def sphere_vn(x, centre, radius):
    """Analytic sphere in float64: v = |x - c| - r, n = (x - c) / |x - c|."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    nrm = np.linalg.norm(d, axis=-1)
    return nrm - radius, d / nrm[..., None]


def sphere_evaluator(points, centre, radius):
    """evaluate() of refine() for the analytic sphere: x = W p in float64.  The Jacobian is the closed form: x cross n =
    (c + d) cross d / |d| = c cross n, which is exactly zero for a sphere at the frame origin (formed numerically from a rounded
    n it is rounding noise instead: see test_registration.py)."""
    points = np.asarray(points, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64)

    def evaluate(W32):
        out = np.zeros((len(W32), SUMS))
        for b, W in enumerate(np.asarray(W32, dtype=np.float64)):
            x = points @ W[:3, :3].T + W[:3, 3]
            v, n = sphere_vn(x, centre, radius)
            out[b] = raw_sums(v, n, x, j=np.concatenate((n, np.cross(centre, n)), axis=-1))
        return out
    return evaluate


def random_twists(B, trans, rot, seed):
    """(B, 6) twists with |u| <= trans and |w| <= rot."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(B, 2, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    mag = rng.uniform(0.3, 1.0, size=(B, 2, 1)) * np.array([trans, rot]).reshape(1, 2, 1)
    return (d * mag).reshape(B, 6)


def perturbed_poses(B, trans, rot, seed, dtype=np.float32):
    """(B, 4, 4) poses Exp(xi) with random twists around the identity."""
    out = np.zeros((B, 4, 4), dtype=dtype)
    eye = np.eye(4)[:3]
    for b, xi in enumerate(random_twists(B, trans, rot, seed)):
        out[b, :3] = retract(eye, xi).astype(dtype)
        out[b, 3, 3] = 1.0
    return out
