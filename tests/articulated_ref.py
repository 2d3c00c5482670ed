"""Float64 numpy restatement of include/pvamd.h "Joint-space normal equations": the twist Jacobian of every leaf, the assembly of
the joint-space normal equations from the per-leaf sums, the brute-force per-point form they must equal, and the
Levenberg-Marquardt step and loop in joint space.  Test infrastructure that shares no code with the product; the chain comes from
tests/fk_ref.py.  The arithmetic is plain float64 (no fused multiply-add): it agrees with the kernels to rounding, the decisions
(winner, activity, Huber branch, accept / reject, failed pivot, zero step, clamp) are the same statements."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import fk_ref as R

SUMS = 28
COUNTS = 5
TRIU = [(r, c) for r in range(6) for c in range(r, 6)]
SURFACE, FREE, OCCUPIED, IGNORE = 0, 1, 2, 3
LAMBDA_MIN = 1e-12
LAMBDA_MAX = 1e12


# ---- the chain as records: what pvamd_chain_twists is given ----
def table_chain(table, leaves=None):
    """(records, origins (F, 4, 4), axes (F, 3)) of a fk_ref table: one record (parent, jtype, jcol, leaf_slot) per
    pvamd_joint_t (fk_ref.expected_records), the float64 origin and the normalised axis of each; a duplicate record (a further
    visual of its link) sits at the identity."""
    records = R.expected_records(table, leaves)
    own, _ = R.frame_records(table, leaves)
    origins = np.tile(np.eye(4), (len(records), 1, 1))
    axes = np.zeros((len(records), 3))
    for row, i in zip(R.frames(table), own):
        origins[i] = R.origin64(row[4], row[5])
        if row[1] is not None and row[2] != R.FIXED:
            k = np.asarray(row[3], dtype=np.float64)
            axes[i] = k / np.linalg.norm(k)
    return records, origins, axes


def _rodrigues(axis, angle):
    """cos I + (1 - cos) a a^T + sin [a]x: the form pvamd_chain_fk states.  For a unit axis it is I + sin K + (1 - cos) K^2; the
    axes of a joint table are float32 values, unit to 6e-8 only, and there the two forms differ by (1 - cos) (1 - |a|^2)."""
    a = np.asarray(axis, dtype=np.float64)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    c = math.cos(angle)
    return c * np.eye(3) + (1.0 - c) * np.outer(a, a) + math.sin(angle) * K


def walk(records, origins, axes, q_row):
    """(F, 4, 4) world_T_record of one configuration: world = world[parent] @ origin @ motion(q)."""
    world = np.zeros((len(records), 4, 4))
    for f, (parent, jtype, jcol, _) in enumerate(records):
        motion = np.eye(4)
        if jtype == 1:
            motion[:3, :3] = _rodrigues(axes[f], float(q_row[jcol]))
        elif jtype == 2:
            motion[:3, 3] = float(q_row[jcol]) * axes[f]
        world[f] = (np.eye(4) if parent < 0 else world[parent]) @ origins[f] @ motion
    return world


def rigid_inverse(m):
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    return out


def stack_and_twists(records, origins, axes, q, offset_inv):
    """T (A, S, 4, 4) = offset_inv[s] @ rigid_inverse(world of leaf s's record) and J (A, S, 6, M): for every moving record k that
    is leaf s's record or an ancestor of it, with a = R(world_k) axis_k and o = t(world_k), xi_W = (o cross a, a) (revolute /
    continuous) or (a, 0) (prismatic), and (R, t) = T_s:  J[:, k] = -(R u_W + t cross (R w_W), R w_W).  Other columns are zero."""
    q = np.asarray(q, dtype=np.float64)
    A, M = q.shape
    S = len(offset_inv)
    slot_record = {r[3]: f for f, r in enumerate(records) if r[3] >= 0}
    T = np.zeros((A, S, 4, 4))
    J = np.zeros((A, S, 6, M))
    for a in range(A):
        world = walk(records, origins, axes, q[a])
        for s in range(S):
            f = slot_record[s]
            Ts = np.asarray(offset_inv[s], dtype=np.float64) @ rigid_inverse(world[f])
            T[a, s] = Ts
            Rm, t = Ts[:3, :3], Ts[:3, 3]
            while f >= 0:
                parent, jtype, jcol, _ = records[f]
                if jtype in (1, 2):
                    ah = world[f][:3, :3] @ axes[f]
                    if jtype == 1:
                        u, w = np.cross(world[f][:3, 3], ah), ah
                    else:
                        u, w = ah, np.zeros(3)
                    J[a, s, :3, jcol] = -(Rm @ u + np.cross(t, Rm @ w))
                    J[a, s, 3:, jcol] = -(Rm @ w)
                f = parent
    return T, J


def ancestors(records, s):
    """The joint columns of the moving records on the way from leaf s's record to the root."""
    f = next(i for i, r in enumerate(records) if r[3] == s)
    cols = []
    while f >= 0:
        if records[f][1] in (1, 2):
            cols.append(records[f][2])
        f = records[f][0]
    return sorted(cols)


def reach(records, origins):
    """Sum of the origins' |xyz| plus 0.3 per prismatic record: how far a frame of the chain can lie from the root."""
    return float(np.abs(origins[:, :3, 3]).sum() + 0.3 * sum(1 for r in records if r[1] == 2))


# ---- the per-pair statements ("Semantic normal equations") ----
def pair_terms(v, n, x, kinds=None, targets=None, delta=math.inf):
    """(terms (N, 28) float64, zero rows for inactive pairs; counts per pair (N, 4): active SURFACE, FREE, OCCUPIED, outlier;
    j (N, 6); weight (N,); r (N,))."""
    v = np.asarray(v).astype(np.float64).reshape(-1)
    n = np.asarray(n).astype(np.float64).reshape(-1, 3)
    x = np.asarray(x).astype(np.float64).reshape(-1, 3)
    N = len(v)
    kinds = np.zeros(N, dtype=np.int64) if kinds is None else np.asarray(kinds).reshape(-1)
    r = v - (0.0 if targets is None else np.asarray(targets).astype(np.float64).reshape(-1))
    with np.errstate(invalid="ignore"):
        active = (kinds == SURFACE) | ((kinds == FREE) & ~(r >= 0.0)) | ((kinds == OCCUPIED) & ~(r <= 0.0))
        a = np.abs(r)
        outlier = active & (a > delta)
        w = np.where(outlier, delta / np.where(outlier, a, 1.0), 1.0)
    j = np.concatenate((n, np.cross(x, n)), axis=-1)
    rho = np.where(outlier, delta * ((a + a) - delta), r * r) if np.isfinite(delta) else r * r
    qv = w * r
    u = w[:, None] * j
    cols = [rho] + [qv * j[:, k] for k in range(6)] + [u[:, rr] * j[:, c] for rr, c in TRIU]
    terms = np.stack(cols, axis=-1)
    terms[~active] = 0.0  # skipped, not multiplied: a NaN of an inactive pair stays out
    flags = np.stack((active & (kinds == SURFACE), active & (kinds == FREE), active & (kinds == OCCUPIED), outlier), axis=-1)
    return terms, flags.astype(np.int64), j, np.where(active, w, 0.0), r


def winners(values):
    """(N,) the first minimum over the leaves of values (S, N), a NaN counting as the minimum."""
    S, N = values.shape
    best = np.full(N, np.inf)
    win = np.zeros(N, dtype=np.int64)
    for s in range(S):
        with np.errstate(invalid="ignore"):
            take = ~(values[s] >= best) & (best == best)
        best = np.where(take, values[s], best)
        win = np.where(take, s, win)
    return win


def fsum_columns(t):
    return np.array([math.fsum(t[:, k]) for k in range(t.shape[1])]) if len(t) else np.zeros(t.shape[1])


def unpack6(sums):
    """(c, g6 (6,), H6 (6, 6)) of 28 sums."""
    H = np.zeros((6, 6))
    for e, (r, c) in enumerate(TRIU):
        H[r, c] = H[c, r] = sums[7 + e]
    return sums[0], np.asarray(sums[1:7]), H


def assemble(leaf_sums, J):
    """cost, g (M,), H (M, M) of one configuration from leaf_sums (S, 28) and J (S, 6, M): sum_s c_s, J_s^T g6_s, J_s^T H6_s J_s."""
    S, _, M = J.shape
    cost, g, H = 0.0, np.zeros(M), np.zeros((M, M))
    for s in range(S):
        c, g6, H6 = unpack6(leaf_sums[s])
        cost = cost + c
        g = g + J[s].T @ g6
        H = H + J[s].T @ H6 @ J[s]
    return cost, g, (H + H.T) / 2 if M else H


def assemble_magnitude(leaf_abs, J):
    """The same products over magnitudes: sum_s |c_s|, |J_s|^T |g6_s|, |J_s|^T |H6_s| |J_s| -- what the rounding errors of the
    factored form scale with (J^T j6 can cancel, so the per-point magnitudes do not bound them)."""
    return assemble(np.abs(leaf_abs), np.abs(J))


def brute_force(terms_j, weights, r, win, J, delta=math.inf):
    """cost, g, H of one configuration summed per point (exactly, math.fsum): j_q = J_{s(p)}^T j6_p, rho, w r j_q, w j_q j_q^T.
    terms_j: (N, 6) j6 per point; weights: (N,) w (0 for inactive pairs); r: (N,); win: (N,) winning leaf."""
    M = J.shape[-1]
    act = weights > 0
    jq = np.einsum("nrm,nr->nm", J[win[act]], terms_j[act])
    w, rr = weights[act], r[act]
    a = np.abs(rr)
    rho = np.where(a > delta, delta * ((a + a) - delta), rr * rr)
    cost = math.fsum(rho)
    g = np.array([math.fsum(w * rr * jq[:, k]) for k in range(M)])
    H = np.array([[math.fsum(w * jq[:, i] * jq[:, k]) for k in range(M)] for i in range(M)]).reshape(M, M)
    return cost, g, H


# ---- a robot of analytic leaves, all float64 ----
@dataclass
class AnalyticRobot:
    """A fk_ref table whose leaves are closed-form fields: leaf_fn[s](x (N, 3) float64) -> (v (N,), n (N, 3))."""
    table: tuple
    leaf_fn: list
    records: list = None
    origins: np.ndarray = None
    axes: np.ndarray = None
    offset_inv: np.ndarray = None

    def __post_init__(self):
        self.records, self.origins, self.axes = table_chain(self.table)
        self.offset_inv = np.stack([rigid_inverse(o) for o in R.visual_offsets64(self.table)])
        assert len(self.leaf_fn) == len(self.offset_inv)

    def leaf_sums(self, q_row, points, kinds=None, targets=None, delta=math.inf):
        """Per leaf the 28 sums (fsum) over the points it wins, the fsum of their magnitudes, the counts, J, and the per-point
        pieces (j6, weights, r, winner) of one configuration."""
        T, J = stack_and_twists(self.records, self.origins, self.axes, np.asarray(q_row, dtype=np.float64)[None], self.offset_inv)
        T, J = T[0], J[0]
        S, N = len(self.leaf_fn), len(points)
        x = np.stack([points @ T[s, :3, :3].T + T[s, :3, 3] for s in range(S)])
        vn = [self.leaf_fn[s](x[s]) for s in range(S)]
        win = winners(np.stack([v for v, _ in vn]))
        idx = np.arange(N)
        xs = x[win, idx]
        vs = np.stack([v for v, _ in vn])[win, idx]
        ns = np.stack([n for _, n in vn])[win, idx]
        terms, flags, j6, w, r = pair_terms(vs, ns, xs, kinds, targets, delta)
        sums = np.stack([fsum_columns(terms[win == s]) for s in range(S)])
        mags = np.stack([fsum_columns(np.abs(terms[win == s])) for s in range(S)])
        leaf_active = np.array([flags[win == s, :3].sum() for s in range(S)])
        return dict(sums=sums, mags=mags, J=J, j6=j6, w=w, r=r, win=win, flags=flags, leaf_active=leaf_active, values=vs)

    def evaluate(self, q, points, kinds=None, targets=None, delta=math.inf):
        """(cost (A,), g (A, M), H (A, M, M)) raw (unscaled) sums of every configuration, the factored form."""
        out = [assemble(e["sums"], e["J"]) for e in (self.leaf_sums(row, points, kinds, targets, delta) for row in np.atleast_2d(q))]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def ellipsoid_fn(center, radii):
    """tests/helpers.AnalyticEllipsoidSDF in numpy float64: v = (|p / r| - 1) min r, n = the normalised p / r^2 (a unit vector; the
    derivative of v only for a sphere)."""
    center, radii = np.asarray(center, dtype=np.float64), np.asarray(radii, dtype=np.float64)

    def fn(x):
        p = (x - center) / radii
        nrm = np.linalg.norm(p, axis=-1)
        g = p / radii
        return (nrm - 1.0) * radii.min(), g / (np.linalg.norm(g, axis=-1, keepdims=True) + 1e-12)
    return fn


# ---- the step and the loop ----
def damped(H, lam):
    A = np.array(H, dtype=np.float64, copy=True)
    for k in range(len(A)):
        d = A[k, k] if A[k, k] > 0.0 else 1.0
        A[k, k] = A[k, k] + lam * d
    return A


def cholesky_solve(A, rhs):
    """(dq, ok): Cholesky without pivoting in the kernel's loop order, any M."""
    M = len(rhs)
    L = np.zeros((M, M))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(M):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (d > 0.0) or not (d < math.inf):
                ok = False
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, M):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        x = np.zeros(M)
        for i in range(M):
            s = rhs[i]
            for k in range(i):
                s = s - L[i, k] * x[k]
            x[i] = s / L[i, i]
        for i in range(M - 1, -1, -1):
            s = x[i]
            for k in range(i + 1, M):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x, ok and bool(np.all(np.isfinite(x)))


@dataclass
class JointState:
    """One configuration of pvamd_joint_lm_step's state."""
    q_try: np.ndarray
    lam: float
    q_acc: np.ndarray = None
    cost_acc: float = math.nan
    g_acc: np.ndarray = None
    H_acc: np.ndarray = None
    accepted: int = 0
    dq: np.ndarray = None
    history: list = field(default_factory=list)  # (q_acc, accepted, bound) after every step
    bound: float = 0.0  # how far the steps so far can lie from exact ones: see lm_step

    def q_next(self):
        return self.q_try.astype(np.float32)


def lm_step(st, cost, g, H, first, up=10., down=0.1, limits=None, lambda_min=LAMBDA_MIN, lambda_max=LAMBDA_MAX):
    if first or cost < st.cost_acc:
        st.q_acc, st.cost_acc, st.g_acc, st.H_acc = st.q_try.copy(), float(cost), np.array(g, copy=True), np.array(H, copy=True)
        st.lam = max(st.lam * down, lambda_min)
        st.accepted += 1
    else:
        st.lam = min(st.lam * up, lambda_max)
    A = damped(st.H_acc, st.lam)
    dq, ok = cholesky_solve(A, -st.g_acc)
    if not ok:
        dq = np.zeros(len(dq))
        st.lam = min(st.lam * up, lambda_max)
    st.dq = dq
    if ok and len(dq):
        # a Cholesky solve is backward stable: within about 2 M (3 M + 1) u cond(A) |dq| of the exact solution (Higham, Accuracy
        # and Stability of Numerical Algorithms, theorem 10.4); twice for two such solves that are compared, twice again for
        # the roundings of the damping and of the right-hand side
        M = len(dq)
        st.bound += 4 * 2 * M * (3 * M + 1) * 2.0 ** -53 * float(np.linalg.cond(A)) * float(np.abs(dq).max())
    if np.all(dq == 0.0):
        st.q_try = st.q_acc.copy()
    else:
        st.q_try = st.q_acc + dq
        if limits is not None:
            st.q_try = np.minimum(np.maximum(st.q_try, limits[:, 0]), limits[:, 1])
    st.history.append((st.q_acc.copy(), st.accepted, st.bound))
    return st


def refine(evaluate, q0, iterations=10, damping=1e-3, up=10., down=0.1, limits=None):
    """refine_joint_configuration's loop.  evaluate((A, M) float32) -> (cost (A,), g (A, M), H (A, M, M)).  Returns the states and
    the initial costs."""
    q0 = np.atleast_2d(np.asarray(q0, dtype=np.float32))
    if limits is not None:
        q0 = np.minimum(np.maximum(q0, limits[:, 0].astype(np.float32)), limits[:, 1].astype(np.float32))
    states = [JointState(q_try=row.astype(np.float64), lam=damping) for row in q0]
    initial = None
    for it in range(iterations + 1):
        cost, g, H = evaluate(np.stack([s.q_next() for s in states]))
        if it == 0:
            initial = np.array(cost, dtype=np.float64, copy=True)
        for a, st in enumerate(states):
            lm_step(st, cost[a], g[a], H[a], it == 0, up, down, limits)
    return states, initial
