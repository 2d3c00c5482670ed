"""Restatements of the trilinear contract (include/pvamd.h "Interpolated queries") for the interpolation tests -- TEST
INFRASTRUCTURE: interp_ref.c compiled on the fly (bit-exact forward, the forward's cell decisions and blend on their own,
float64 per-point VJP) and a float64 torch restatement that autograd differentiates given the kernel's decisions."""
import ctypes

import numpy as np
import torch

from tests import c_ref


def load():
    return c_ref.load("interp_ref")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def grid_numbers(cached, f64):
    """(records [n][4] float32, shape int32[3], min, res) of a CachedSDF in the query dtype's statement."""
    v = cached._view
    rec = np.ascontiguousarray(cached._packed.detach().cpu().numpy().astype(np.float32))
    shape = np.array(v.shape, dtype=np.int32)
    if f64:
        return rec, shape, np.array([float(x) for x in v.dmin], np.float64), np.array([float(x) for x in v.dres], np.float64)
    return rec, shape, np.array([float(x) for x in v.fmin], np.float32), np.array([float(x) for x in v.fres], np.float32)


def forward(rec, shape, mn, res, pts, valid):
    """val, grad of the in-range points (others NaN): float32 or float64 by pts' dtype."""
    pts = np.ascontiguousarray(pts)
    f64 = pts.dtype == np.float64
    P = pts.shape[0]
    val = np.full((P,), np.nan, pts.dtype)
    grad = np.full((P, 3), np.nan, pts.dtype)
    valid = np.ascontiguousarray(valid.astype(np.uint8))
    fn = load().interp_forward_f64 if f64 else load().interp_forward_f32
    fn(_p(rec), _p(shape), _p(np.ascontiguousarray(mn, pts.dtype)), _p(np.ascontiguousarray(res, pts.dtype)), _p(pts),
       ctypes.c_int64(P), _p(valid), _p(val), _p(grad))
    return val, grad


def cell(shape, mn, res, pts):
    """The forward's cell decisions per point, in pts' dtype (float32 / float64): (i (P, 3) int32, f (P, 3), clamped (P, 3) bool).
    The signature oracle.conditioned_vjp's trilinear mode asks of its cell function."""
    pts = np.ascontiguousarray(pts)
    assert pts.dtype in (np.float32, np.float64)
    f64 = pts.dtype == np.float64
    P = pts.shape[0]
    idx = np.zeros((P, 3), np.int32)
    frac = np.zeros((P, 3), pts.dtype)
    cl = np.zeros((P, 3), np.uint8)
    fn = load().interp_cell_f64 if f64 else load().interp_cell_f32
    fn(_p(np.ascontiguousarray(shape, np.int32)), _p(np.ascontiguousarray(mn, pts.dtype)), _p(np.ascontiguousarray(res, pts.dtype)),
       _p(pts), ctypes.c_int64(P), _p(idx), _p(frac), _p(cl))
    return idx, frac, cl.astype(bool)


def blend(rec, shape, idx, frac):
    """(val, grad) of the forward's lerp sequence for given cell decisions, in frac's dtype."""
    frac = np.ascontiguousarray(frac)
    f64 = frac.dtype == np.float64
    P = frac.shape[0]
    val = np.empty((P,), frac.dtype)
    grad = np.empty((P, 3), frac.dtype)
    fn = load().interp_blend_f64 if f64 else load().interp_blend_f32
    fn(_p(rec), _p(np.ascontiguousarray(shape, np.int32)), _p(np.ascontiguousarray(idx, np.int32)), _p(frac), ctypes.c_int64(P),
       _p(val), _p(grad))
    return val, grad


def vjp(rec, shape, mn, res, pts, valid, dval, dgrad):
    pts = np.ascontiguousarray(pts, np.float64)
    P = pts.shape[0]
    out = np.full((P, 3), np.nan, np.float64)
    load().interp_vjp_f64(_p(rec), _p(shape), _p(np.ascontiguousarray(mn, np.float64)), _p(np.ascontiguousarray(res, np.float64)),
                          _p(pts), ctypes.c_int64(P), _p(np.ascontiguousarray(valid.astype(np.uint8))),
                          _p(np.ascontiguousarray(dval, np.float64)), _p(np.ascontiguousarray(dgrad, np.float64)), _p(out))
    return out


# ---------------------------------------------------------------- float64 torch (autograd) restatement
def leaf_torch(cached, x, inside):
    """(val, grad) of one trilinear BOUNDING_BOX leaf at leaf-frame points x (..., 3) float64, differentiable w.r.t. x: in range
    (the given decision) the interpolation, outside the reference's bounding-box statements (sdf.py:559-571)."""
    v = cached._view
    dev = x.device
    rec = cached._packed.detach().to(device=dev, dtype=torch.float64)
    shape = torch.tensor(v.shape, device=dev)
    mn = torch.tensor([float(a) for a in v.dmin], dtype=torch.float64, device=dev)
    res = torch.tensor([float(a) for a in v.dres], dtype=torch.float64, device=dev)
    s = (x - mn) / res
    c = torch.maximum(torch.minimum(s, (shape - 1).to(torch.float64)), torch.zeros_like(s))
    i = torch.minimum(torch.floor(c.detach()), (shape - 2).to(torch.float64)).clamp_min(0).long()
    f = c - i.to(torch.float64)
    ny, nz = v.shape[1], v.shape[2]

    def R(a, b, e):
        flat = ((i[..., 0] + a) * ny + (i[..., 1] + b)) * nz + (i[..., 2] + e)
        return rec[flat.clamp(0, rec.shape[0] - 1)]

    def lerp(a, b, t):
        return a + t.unsqueeze(-1) * (b - a)

    e = [lerp(R(a, b, 0), R(a, b, 1), f[..., 2]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]
    out = lerp(lerp(e[0], e[1], f[..., 1]), lerp(e[2], e[3], f[..., 1]), f[..., 0])
    bb = cached.bb.to(device=dev, dtype=torch.float64)
    lo = (bb[:, 0] - x).clamp_min(0)
    hi = (x - bb[:, 1]).clamp_min(0)
    d = torch.where(bb[:, 0] - x > 0, -(lo + hi), lo + hi)
    n = d.norm(dim=-1)
    ins = inside.to(dev)
    val = torch.where(ins, out[..., 0], n)
    safe = torch.where(ins, torch.ones_like(n), n)
    grad = torch.where(ins.unsqueeze(-1), out[..., 1:], d / safe.unsqueeze(-1))
    return val, grad


def composed_torch(leaves, m, pts, leaf_ids, insides):
    """Composed forward in float64 torch given the kernel's winners: m (S*A, 4, 4) leaf-major, pts (P, 3), leaf_ids (A, P),
    insides (S, A, P) the per-leaf range decisions.  Returns (A, P), (A, P, 3)."""
    S = len(leaves)
    A = m.shape[0] // S
    m = m.reshape(S, A, 4, 4)
    vals, grads = [], []
    for s, c in enumerate(leaves):
        L, t = m[s, :, :3, :3], m[s, :, :3, 3]
        x = pts.unsqueeze(0) @ L.transpose(-1, -2) + t.unsqueeze(1)  # (A, P, 3)
        v, g = leaf_torch(c, x, insides[s])
        vals.append(v)
        grads.append(g @ L)  # L^T g per configuration
    V, G = torch.stack(vals), torch.stack(grads)
    idx = leaf_ids.long().to(V.device).unsqueeze(0)
    val = V.gather(0, idx).squeeze(0)
    grad = G.gather(0, idx.unsqueeze(-1).expand(1, *G.shape[1:])).squeeze(0)
    return val, grad
