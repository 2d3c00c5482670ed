"""Float64 numpy restatement of include/pvamd.h "Semantic normal equations": the per-pair statements (residual against a target,
the activity of a pair under its point's kind, the Huber branch) on top of tests/registration_ref.py, whose Jacobian, step and
loop it uses as they are.  Test infrastructure: the product never imports it.  Plain float64 (no fused multiply-add): the sums
agree with the kernels to rounding; the decisions are single IEEE operations on the same inputs and agree exactly."""
import numpy as np

from tests import registration_ref as R

SURFACE, FREE, OCCUPIED, IGNORE = 0, 1, 2, 3
COUNTS = 5
# The c of the sums' bound (N + c) 2^-53 fsum |terms|, counted from the roundings inside an outlier term: w = delta / a (1), then
# q = w r or u = w j (1), the cost term's (a + a) - delta (1; a + a is exact), and the term's final product, which this
# restatement rounds and the kernel's fused multiply-add does not (1): 4.  The first three are the same IEEE operations on the
# same inputs on both sides; they are counted as if they were not.  An inlier term has the last one only.  The N stands for the
# N - 1 additions of a sum of N terms in any fixed order and the one spare unit covers the second-order terms.
BOUND_C = 4


def residual(v, targets):
    """r = (double)v - (double)s in the shape of v: one rounding (exact for float32 inputs unless the exponents lie far apart)."""
    v = np.asarray(v).astype(np.float64)
    if targets is None:
        return v - 0.0
    return v - np.asarray(targets, dtype=np.float32).astype(np.float64)


def activity(r, kinds):
    """(boolean active in the shape of r, kinds as int64): the contract's inactive cases negated, so a NaN r of a kind 0, 1 or 2
    is active.  kinds: any integers, broadcast against r; what is not 0, 1 or 2 is IGNORE."""
    if kinds is None:
        return np.ones(r.shape, dtype=bool), np.zeros(r.shape, dtype=np.int64)
    kinds = np.broadcast_to(np.asarray(kinds).astype(np.int64), r.shape)
    with np.errstate(invalid="ignore"):
        inactive = ((kinds < SURFACE) | (kinds >= IGNORE)) | ((kinds == FREE) & (r >= 0.0)) | ((kinds == OCCUPIED) & (r <= 0.0))
    return ~inactive, kinds


def sem_counts(v, kinds, targets, delta, in_range):
    """The five counts (..., 5) of poses' values v (..., N) at once; kinds, targets (N,), in_range (..., N)."""
    r = residual(v, targets)
    active, kinds = activity(r, kinds)
    with np.errstate(invalid="ignore"):
        outlier = active & (np.abs(r) > delta)
    cols = [np.asarray(in_range, dtype=bool)] + [active & (kinds == k) for k in (SURFACE, FREE, OCCUPIED)] + [outlier]
    return np.stack([c.sum(-1) for c in cols], axis=-1).astype(np.int64)


def sem_terms(v, n, x, kinds=None, targets=None, delta=np.inf, j=None, in_range=None):
    """((N, 28) float64 terms of one pose with the rows of inactive pairs zero, the five counts).  in_range: boolean (N,) of the
    query's range decision (None: every point, as on the generic path)."""
    r = residual(np.asarray(v).reshape(-1), None if targets is None else np.asarray(targets).reshape(-1))
    N = r.shape[0]
    j = (R.jacobian(x, n) if j is None else np.asarray(j, dtype=np.float64)).reshape(-1, 6)
    active, kinds = activity(r, None if kinds is None else np.asarray(kinds).reshape(-1))
    a = np.abs(r)
    with np.errstate(invalid="ignore"):
        outlier = active & (a > delta)
    t = np.zeros((N, R.SUMS))
    with np.errstate(all="ignore"):
        w = np.where(outlier, delta / a, 1.0)  # times one is exact: an inlier enters as (r, j)
        q = w * r
        u = w[:, None] * j
        cols = [np.where(outlier, delta * ((a + a) - delta), r * r)] + [q * j[:, k] for k in range(6)] + \
               [u[:, rr] * j[:, cc] for rr, cc in R.TRIU]
    full = np.stack(cols, axis=-1)
    t[active] = full[active]  # selected, not multiplied by zero: an inactive pair's NaN stays out
    counts = np.array([N if in_range is None else int(np.asarray(in_range).sum()), int((active & (kinds == SURFACE)).sum()),
                       int((active & (kinds == FREE)).sum()), int((active & (kinds == OCCUPIED)).sum()), int(outlier.sum())],
                      dtype=np.int64)
    return t, counts


def sem_raw_sums(v, n, x, kinds=None, targets=None, delta=np.inf, j=None):
    t, counts = sem_terms(v, n, x, kinds, targets, delta, j)
    return t.sum(axis=0), counts


def sem_sphere_evaluator(points, centre, radius, kinds=None, targets=None, delta=np.inf):
    """evaluate() of registration_ref.refine() for the analytic sphere under the semantic contract (x = W p in float64, the
    closed-form Jacobian of registration_ref.sphere_evaluator).  evaluate.counts holds the (B, 5) counts of its last call."""
    points = np.asarray(points, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64)

    def evaluate(W32):
        out = np.zeros((len(W32), R.SUMS))
        evaluate.counts = np.zeros((len(W32), COUNTS), dtype=np.int64)
        for b, W in enumerate(np.asarray(W32, dtype=np.float64)):
            x = points @ W[:3, :3].T + W[:3, 3]
            v, n = R.sphere_vn(x, centre, radius)
            out[b], evaluate.counts[b] = sem_raw_sums(v, n, x, kinds, targets, delta,
                                                      j=np.concatenate((n, np.cross(centre, n)), axis=-1))
        return out
    evaluate.counts = None
    return evaluate
