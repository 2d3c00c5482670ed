"""Decision-conditioned float64 VJP of the cached, composed and grid-chamfer queries -- TEST INFRASTRUCTURE ONLY.

The backward kernels (pytorch_volumetric_amd/csrc/backward.hip) promise the gradient torch autograd gives through the
reference's expressions (sdf.py:399,409,421-426,556-571; chamfer.py:82-94) GIVEN THE FORWARD'S DECISIONS: the winning leaf,
the range test, the voxel and the active box axes.  This module takes those decisions from the C oracle (bit-exact with the
forward kernels) and differentiates the same expressions in float64 with torch autograd:

  * the leaf-frame point is the forward's own x (oracle.transform_pairs: the kernels' fma chain), entered straight-through,
    x = (L p + t) + (x_fwd - (L p + t)).detach(), so the box branch is evaluated exactly where the kernel evaluated it
    (a point 1 ulp outside a face has |d| ~ 1e-7: float64-vs-float32 differences in x would move n by 10 %);
  * in range: v and g are the record's (constants, no derivative w.r.t. x);
  * out of range: d = signed excess over the surface box on the forward's active axes (bb - x > 0 / x - bb > 0 on the
    float32 box for float32 points, the float64 box for float64 points), zero elsewhere; v = |d|, g = d / |d|;
  * the gradient goes back as gg = L^T g (the transpose form the README states for raw matrix entries), so all 12 entries
    of dtf compare directly and row 3 is exactly zero;
  * chamfer: (scale v)^2 summed per transform (the division by N happens outside, in torch).

Besides the VJP, every function returns, per output entry, sum |term|: the sum over the pairs feeding that entry of the
magnitude of the pair's contribution, taken over the kernel's own intermediate products (|L| |dgg|, |n_d| (|n| . |dg|),
...), so that the rounding of a kernel that computes the same expressions in another order is bounded by
k eps sum|term| whatever cancels.

The trilinear mode (interpolation="trilinear"; composed_vjp / cached_vjp with `interp`; tests/test_interp_edges_gpu.py, as
tests/test_autograd_edges_gpu.py is the nearest mode's) holds the trilinear forward's decisions the same way.  The winner is
the trilinear forward's (tests/interp_ref.c composed_forward_f32 / _f64, handed in as `leaf`), the range test is the nearest
mode's (the C oracle, as above), and for an in-range pair the cell i, the fractions f and the clamped flags come from a cell
function that runs the forward's statements in the forward's dtype on the forward's x (tests/interp_ref.c interp_cell_f32 /
_f64); none of them is re-derived in float64, and no floor, minimum or maximum is differentiated:
  * in range: (v, g) = the blend of the eight records R[i + (a, b, e)] with the weights f or 1 - f per axis, in float64, at
    f = f_fwd + (xs - x_fwd) / res (1 - clamped): the value is the forward's fraction, the derivative 1 / res, exactly 0 on a
    clamped axis (include/pvamd.h "Interpolated queries": clamped means c != s, otherwise the full derivative -- at an integer s
    the upper cell's, at s == n - 1 cell n - 2's with f = 1);
  * out of range, gg = L^T g and the matrix gradient: as above.
Its magnitudes: with u = (dv, L dgg) and |u| = (|dv|, |L| |dgg|), dx_mag_d = (1 - clamped_d) / res_d sum_q |u_q| sum over the
eight corners of (the product of the OTHER two axes' weights) |R_q(corner)| -- every difference b - a along axis d replaced
by |a| + |b|, which, f lying in [0, 1], covers the kernel's lerps and differences whatever cancels; exactly 0 on a clamped
axis, so the bound demands an exact zero there.  The gr magnitude is the same blend (all three axes' weights) of |R|; dp_mag
and dtf_mag follow from dx_mag and gr_mag as above.
"""
import numpy as np
import torch

from oracle import oracle


def _decisions(grids, tf, A, pts, leaf):
    """x (A,P,3) in the forward's dtype, oob (A,P), record gradient (A,P,3) f64, box lo/hi per pair (A,P,3) f64."""
    f64 = pts.dtype == np.float64
    x = oracle.transform_pairs(tf, A, pts, leaf)
    P = pts.shape[0]
    oob = np.zeros((A, P), bool)
    rec = np.zeros((A, P, 3), np.float64)
    lo = np.zeros((A, P, 3), np.float64)
    hi = np.zeros((A, P, 3), np.float64)
    for s, g in enumerate(grids):
        m = leaf == s
        if not m.any():
            continue
        query = oracle.cached_query_f64 if f64 else oracle.cached_query
        _, gr, out = query(g, x[m])
        oob[m] = out
        rec[m] = np.where(out[:, None], 0.0, gr)
        c = g.c
        lo[m] = np.array(c.dbb_min[:] if f64 else c.bb_min[:], np.float64)
        hi[m] = np.array(c.dbb_max[:] if f64 else c.bb_max[:], np.float64)
    return x, oob, rec, lo, hi


def _segment_sum(t, key, nkeys):
    """sum of t[i] over i with key[i] == k, for k < nkeys: (nkeys, ...) float64, pairwise (cascade) summation per segment."""
    out = torch.zeros((nkeys,) + tuple(t.shape[1:]), dtype=torch.float64)
    if t.shape[0] == 0:
        return out
    order = torch.argsort(key, stable=True)
    ts = t[order].reshape(t.shape[0], -1)
    keys, counts = torch.unique_consecutive(key[order], return_counts=True)
    start = 0
    for k, n in zip(keys.tolist(), counts.tolist()):
        # an inner-dimension reduction of a contiguous tensor: torch sums it in cascade (error ~ log n eps)
        out[k] = ts[start:start + n].t().contiguous().sum(dim=1).reshape(t.shape[1:])
        start += n
    return out


def _corner_records(rec, shape, i):
    """The eight corner records of the cells i (P, 3): (P, 2, 2, 2, 4) float64, [a][b][e] = R[i+a, j+b, k+e]."""
    ny, nz = int(shape[1]), int(shape[2])
    i = i.astype(np.int64)
    out = np.empty((i.shape[0], 2, 2, 2, 4), np.float64)
    for a in (0, 1):
        for b in (0, 1):
            for e in (0, 1):
                out[:, a, b, e] = rec[((i[:, 0] + a) * ny + (i[:, 1] + b)) * nz + (i[:, 2] + e)]
    return out


def _interp_decisions(interp, x, leaf, oob):
    """The forward's cell decisions of the in-range pairs, per pair: corner records (A,P,2,2,2,4) f64, fractions (A,P,3) f64
    (the forward dtype's bits), clamped (A,P,3), resolution (A,P,3) f64 in the forward's statement."""
    numbers, cell = interp
    A, P = leaf.shape
    R = np.zeros((A, P, 2, 2, 2, 4), np.float64)
    f = np.zeros((A, P, 3), np.float64)
    cl = np.zeros((A, P, 3), bool)
    res = np.ones((A, P, 3), np.float64)
    for s, (rec, shape, mn, rs) in enumerate(numbers):
        m = (leaf == s) & ~oob
        if not m.any():
            continue
        i, fr, c = cell(shape, mn, rs, np.ascontiguousarray(x[m]))
        assert fr.dtype == x.dtype, "the cell function must answer in the forward's dtype"
        R[m] = _corner_records(np.asarray(rec, np.float64), shape, i)
        f[m], cl[m], res[m] = fr, c, np.asarray(rs, np.float64)
    return R, f, cl, res


def _blend(R, w):
    """sum over the corners of w_x w_y w_z R: R (P,2,2,2,Q), w a list of three (P,2) weight pairs -> (P,Q)."""
    return torch.einsum("pa,pb,pe,pabeq->pq", w[0], w[1], w[2], R)


def composed_vjp(grids, tf, A, pts, dval=None, dgrad=None, leaf=None, chamfer_scale=None, interp=None):
    """VJP of ComposedSDF.__call__ over the leaves `grids` (list of S oracle.Grid) given the forward's decisions.

    tf: (S*A, 4, 4) obj->leaf stack, leaf-major, in the dtype the kernels read (float32, or float64 for float64 points);
    pts: (P, 3) float32 / float64 (selects the float32 / float64 forward); dval (A, P) / dgrad (A, P, 3): the upstream, or
    None; leaf: the forward's winner per pair (A, P) -- from the oracle when None.
    chamfer_scale: the grid-chamfer backward instead (S = 1, every pair on leaf 0, dval = the (B,) upstream of the sums of
    (scale v)^2, dgrad unused).
    interp: the trilinear mode (module docstring): (numbers, cell) -- numbers[s] = (records [n][4] float32, shape, min, res) of
    leaf s in the query dtype's statement, cell(shape, min, res, x) -> (i, f, clamped) per point by the forward's statements in
    x's dtype (tests/interp_ref.py: grid_numbers, cell).  `leaf` must then be given: the trilinear forward's winners.
    Returns dict(dpoints (P,3), dtf (S*A,4,4), dpoints_mag, dtf_mag, leaf (A,P), oob (A,P)), float64 torch on the CPU."""
    pts = np.ascontiguousarray(np.asarray(pts))
    f64 = pts.dtype == np.float64
    if not f64:
        pts = pts.astype(np.float32)
    tf = np.ascontiguousarray(np.asarray(tf), dtype=np.float64 if f64 else np.float32).reshape(-1, 4, 4)
    S, P = len(grids), pts.shape[0]
    assert tf.shape[0] == S * A
    if leaf is None:
        assert interp is None, "the trilinear mode takes its winners from the trilinear forward's restatement"
        if chamfer_scale is not None:
            leaf = np.zeros((A, P), np.int32)
        else:
            leaf = (oracle.composed_query_f64 if f64 else oracle.composed_query)(grids, tf, A, pts)[2]
    leaf = np.ascontiguousarray(leaf, dtype=np.int32).reshape(A, P)
    x, oob, rec, bblo, bbhi = _decisions(grids, tf, A, pts, leaf)
    if interp is not None:
        assert chamfer_scale is None and len(interp[0]) == S
        cR, cf, ccl, cres = _interp_decisions(interp, x, leaf, oob)

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    tf64, p64 = T(tf), T(pts)
    up_v = None if dval is None else torch.as_tensor(dval).detach().cpu().to(torch.float64)
    up_g = None if dgrad is None or chamfer_scale is not None else \
        torch.as_tensor(dgrad).detach().cpu().to(torch.float64).reshape(A, P, 3)
    if up_v is not None and chamfer_scale is None:
        up_v = up_v.reshape(A, P)
    dp = torch.zeros(P, 3, dtype=torch.float64)
    dp_mag = torch.zeros(P, 3, dtype=torch.float64)
    dtf = torch.zeros(S * A, 4, 4, dtype=torch.float64)
    dtf_mag = torch.zeros(S * A, 4, 4, dtype=torch.float64)
    for a in range(A):  # one configuration at a time: (P, 4, 4) per-pair copies of the matrices
        lf = torch.from_numpy(leaf[a].astype(np.int64))
        sa = lf * A + a
        pp = p64.clone().requires_grad_()
        MM = tf64[sa].clone().requires_grad_()
        L, t = MM[:, :3, :3], MM[:, :3, 3]
        xl = (L @ pp.unsqueeze(-1)).squeeze(-1) + t
        xs = xl + (T(x[a]) - xl).detach()  # straight-through: the value is the forward's x, the derivative that of L p + t
        out = torch.from_numpy(oob[a])
        lo_b, hi_b = T(bblo[a]), T(bbhi[a])
        lo_act = (lo_b > T(x[a])) & out[:, None]
        hi_act = (T(x[a]) > hi_b) & out[:, None]
        d = torch.where(lo_act, -(lo_b - xs), torch.where(hi_act, xs - hi_b, torch.zeros_like(xs)))  # sdf.py:559-567
        sq = (d * d).sum(-1)
        ok = out & (sq > 0)
        nrm = torch.sqrt(torch.where(ok, sq, torch.ones_like(sq)))
        n = torch.where(ok[:, None], d / nrm[:, None], torch.full_like(d, float("nan")))  # 0 / 0 where the box is not left
        v = torch.where(ok, nrm, torch.zeros_like(nrm))  # in range: a record value, no derivative
        g = torch.where(out[:, None], n, T(rec[a]))
        if interp is not None:
            # in range: the blend of the eight records at the forward's fractions (straight-through: the value is the forward's
            # f, the derivative 1 / res, 0 on a clamped axis); no floor, minimum or maximum is differentiated
            Ra, keep = T(cR[a]), T(~ccl[a])
            fs = T(cf[a]) + ((xs - T(x[a])) / T(cres[a])) * keep
            w3 = [torch.stack((1 - fs[:, d], fs[:, d]), dim=1) for d in range(3)]
            o = _blend(Ra, w3)
            v = torch.where(out, v, o[:, 0])
            g = torch.where(out[:, None], n, o[:, 1:])
        gg = (L.transpose(-1, -2) @ g.unsqueeze(-1)).squeeze(-1)  # gg = L^T g
        loss = torch.zeros((), dtype=torch.float64)
        dv_mag = torch.zeros(P, dtype=torch.float64)
        dgg = torch.zeros(P, 3, dtype=torch.float64)
        if chamfer_scale is not None:
            if up_v is not None:
                loss = loss + up_v[a] * ((chamfer_scale * v) ** 2).sum()
                dv_mag = (up_v[a].abs() * 2 * chamfer_scale * chamfer_scale) * v.detach()
        else:
            if up_v is not None:
                loss = loss + (up_v[a] * v).sum()
                dv_mag = up_v[a].abs()
            if up_g is not None:
                dgg = up_g[a]
                loss = loss + (dgg * gg).sum()
        if not loss.requires_grad:
            continue
        gp, gM = torch.autograd.grad(loss, (pp, MM), allow_unused=True)
        gp = torch.zeros_like(pp) if gp is None else gp
        gM = torch.zeros_like(MM) if gM is None else gM
        # magnitudes of the kernel's own intermediate products (backward.hip: dg = L dgg, dx, dp = L^T dx, dtf terms)
        with torch.no_grad():
            Lm, nm = L.detach().abs(), torch.nan_to_num(n.detach()).abs()
            dg_m = (Lm @ dgg.abs().unsqueeze(-1)).squeeze(-1)
            nrm_d = torch.where(ok, nrm.detach(), torch.ones_like(sq))
            act = lo_act | hi_act
            dx_m = dv_mag[:, None] * nm
            if chamfer_scale is None:
                dx_m = dx_m + (dg_m + nm * (nm * dg_m).sum(-1, keepdim=True)) / nrm_d[:, None]
            dx_m = torch.where(act & ok[:, None], dx_m, torch.zeros_like(dx_m))
            gr_m = torch.where(out[:, None], nm, T(rec[a]).abs()) if chamfer_scale is None else torch.zeros_like(nm)
            if interp is not None:
                w0 = [w.detach() for w in w3]
                one = [torch.ones_like(w) for w in w0]
                u_m = torch.cat((dv_mag[:, None], dg_m), dim=1)  # |u_q|: (|dv|, |L| |dgg|)
                Rm = Ra.abs()
                in_m = torch.stack([(_blend(Rm, [one[e] if e == d else w0[e] for e in range(3)]) * u_m).sum(-1)
                                    for d in range(3)], dim=1) * keep / T(cres[a])
                dx_m = torch.where(out[:, None], dx_m, in_m)
                gr_m = torch.where(out[:, None], nm, _blend(Rm, w0)[:, 1:])
            dp_m = (Lm.transpose(-1, -2) @ dx_m.unsqueeze(-1)).squeeze(-1)
            tf_m = torch.zeros(P, 4, 4, dtype=torch.float64)
            tf_m[:, :3, :3] = dx_m.unsqueeze(-1) * p64.abs().unsqueeze(1) + gr_m.unsqueeze(-1) * dgg.abs().unsqueeze(1)
            tf_m[:, :3, 3] = dx_m
        dp += gp
        dp_mag += dp_m
        dtf += _segment_sum(gM, sa, S * A)
        dtf_mag += _segment_sum(tf_m, sa, S * A)
    return dict(dpoints=dp, dtf=dtf, dpoints_mag=dp_mag, dtf_mag=dtf_mag, leaf=torch.from_numpy(leaf), oob=torch.from_numpy(oob))


def cached_vjp(grid, pts, dval=None, dgrad=None, interp=None):
    """VJP of CachedSDF.__call__ (one leaf, the identity frame): dict(dpoints, dpoints_mag, oob).  interp: composed_vjp's, for
    the one leaf."""
    pts = np.asarray(pts)
    eye = np.eye(4, dtype=pts.dtype if pts.dtype == np.float64 else np.float32)[None]
    P = pts.shape[0]
    r = composed_vjp([grid], eye, 1, pts, None if dval is None else torch.as_tensor(dval).reshape(1, P),
                     None if dgrad is None else torch.as_tensor(dgrad).reshape(1, P, 3), leaf=np.zeros((1, P), np.int32),
                     interp=interp)
    return dict(dpoints=r["dpoints"], dpoints_mag=r["dpoints_mag"], oob=r["oob"][0])


def chamfer_vjp(grid, W, pts, scale, dsum):
    """VJP of the per-transform sums of (scale v)^2 (GridChamfer): dsum (B,) upstream of the sums.
    dict(dW (B,4,4), dpoints (N,3), dW_mag, dpoints_mag)."""
    W = np.asarray(W, dtype=np.float32).reshape(-1, 4, 4)
    r = composed_vjp([grid], W, W.shape[0], np.asarray(pts, dtype=np.float32), dval=torch.as_tensor(dsum).reshape(-1),
                     chamfer_scale=float(scale))
    return dict(dW=r["dtf"], dpoints=r["dpoints"], dW_mag=r["dtf_mag"], dpoints_mag=r["dpoints_mag"])


def within_bound(got, want, mag, unit, n_chain, c=4.0, tiny=0.0):
    """|got - want| <= c unit (n_chain + 8) mag + tiny, elementwise; NaN only where both are NaN.  Returns (ok, worst ratio,
    index of the worst entry) for the message."""
    got = got.detach().cpu().to(torch.float64)
    want, mag = want.to(torch.float64), mag.to(torch.float64)
    n_chain = torch.as_tensor(n_chain, dtype=torch.float64)
    bound = c * unit * (n_chain + 8) * mag + tiny
    both_nan = torch.isnan(got) & torch.isnan(want)
    err = torch.where(both_nan, torch.zeros_like(got), (got - want).abs())
    err = torch.nan_to_num(err, nan=float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = int(torch.argmax(ratio.reshape(-1))) if ratio.numel() else 0
    return bool((err <= bound).all()), float(ratio.max()) if ratio.numel() else 0.0, worst
