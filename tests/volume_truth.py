"""Float64 references of the volume pipeline for its tests -- TEST INFRASTRUCTURE: what the contract's float32 statements
(include/pvamd.h "Ray integration", "TSDF integration") approximate, in plain numpy over all voxels of a lattice, and the bounds
within which a float32 evaluation must stay.  The C restatements (tests/*_ref.c) say WHICH float32 result is right; these say
that the restatements themselves are geometrically right."""
import numpy as np


def lattice64(lat):
    """(fmin (3,), fres (3,), shape) of a lattice: its float32 fields taken as doubles."""
    return np.array(list(lat.fmin), np.float64), np.array(list(lat.fres), np.float64), tuple(lat.shape)


# ---------------------------------------------------------------- the walk against the segment
def walk_bounds(lat, o, e, max_range=np.inf, eps=1e-3):
    """(must, may): two (nx, ny, nz) bool arrays, the cells a walk of the ray o -> e has to visit and the cells it may visit.
    Lattice coordinates a = (o - fmin) / fres and likewise for e, in float64; the segment is a + t * d over [0, t1],
    t1 = min(1, max_range / |e - o|).  Per cell c the slab method gives the parameter interval of the segment inside the box
    [c - 0.5 - g, c + 0.5 + g]: `must` holds the cells whose interval for g = -eps has a chord longer than eps voxels, `may` the
    cells whose interval for g = +eps is not empty.  Finite rays only."""
    fmin, fres, shape = lattice64(lat)
    o, e = np.asarray(o, np.float32).astype(np.float64), np.asarray(e, np.float32).astype(np.float64)
    a, d = (o - fmin) / fres, (e - fmin) / fres - (o - fmin) / fres
    length = np.linalg.norm(e - o)
    t1 = max_range / length if length > max_range else 1.0

    def interval(g):
        enter, leave = np.zeros(shape), np.full(shape, t1)
        for k in range(3):
            c = np.arange(shape[k], dtype=np.float64)
            lo, hi = c - 0.5 - g, c + 0.5 + g
            if d[k] == 0.0:
                inside = (lo <= a[k]) & (a[k] <= hi)
                near, far = np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)
            else:
                u, w = (lo - a[k]) / d[k], (hi - a[k]) / d[k]
                near, far = np.minimum(u, w), np.maximum(u, w)
            view = [None, None, None]
            view[k] = slice(None)
            enter, leave = np.maximum(enter, near[tuple(view)]), np.minimum(leave, far[tuple(view)])
        return enter, leave

    enter, leave = interval(-eps)
    with np.errstate(invalid="ignore"):  # a ray of no length: (-inf) * 0, and NaN > eps is False
        must = (leave - enter) * np.linalg.norm(d) > eps
    enter, leave = interval(eps)
    return must, enter <= leave


def check_walks(lat, origins, endpoints, max_range, cells_of, eps=1e-3):
    """must <= walked <= may (walk_bounds) for every ray, none left out; a ray with a non-finite coordinate visits nothing.
    cells_of(o, e, max_range): the (m, 3) voxel indices one ray visits, in any order.  Returns (cells walked, cells of `must`),
    summed over the rays."""
    shape = tuple(lat.shape)
    walked_total = must_total = 0
    for i, (o, e) in enumerate(zip(origins, endpoints)):
        cells = np.asarray(cells_of(o, e, max_range)).reshape(-1, 3)
        walked = np.zeros(shape, bool)
        walked[tuple(cells.T)] = True
        if not (np.isfinite(o).all() and np.isfinite(e).all()):
            assert not walked.any(), (i, o, e)
            continue
        must, may = walk_bounds(lat, o, e, max_range, eps)
        missed, extra = must & ~walked, walked & ~may
        assert not missed.any() and not extra.any(), (i, o.tolist(), e.tolist(), max_range, np.argwhere(missed)[:4].tolist(),
                                                     np.argwhere(extra)[:4].tolist())
        walked_total += int(walked.sum())
        must_total += int(must.sum())
    return walked_total, must_total


# ---------------------------------------------------------------- TSDF integration
def tsdf_integrate64(lat, depth, inverse, intrinsics, truncation, max_depth=np.inf, weight=1.0, max_weight=np.inf,
                     pixel_tol=1e-3, length_tol=None):
    """Statements 2-9 of "TSDF integration" in float64 on a fresh volume, vectorised over the voxels.  The inputs are the
    float32 numbers the kernel is handed (lattice fields, depth (K, H, W), inverse (K, 3, 4), the scalars), taken as doubles.
    Returns (state (nx, ny, nz, 2) float64, updated (nx, ny, nz) bool, undecided (nx, ny, nz) bool).  A voxel is undecided when,
    in some frame, a comparison it reaches is closer to its threshold than pixel_tol (u and v against the image's ends and the
    pixel boundaries, in pixels) or length_tol (p_z > 0 and sdf >= -truncation, in world units): a float32 evaluation may
    decide it either way."""
    fmin, fres, shape = lattice64(lat)
    f32 = lambda v: float(np.float32(v))
    fx, fy, cx, cy = (f32(v) for v in intrinsics)
    truncation, max_depth, weight, max_weight = f32(truncation), f32(max_depth), f32(weight), f32(max_weight)
    depth = np.asarray(depth, np.float32).astype(np.float64)
    depth = depth[None] if depth.ndim == 2 else depth
    inverse = np.asarray(inverse, np.float32).astype(np.float64).reshape(-1, 3, 4)
    K, H, W = depth.shape
    assert inverse.shape[0] == K and length_tol is not None
    axes = [fmin[k] + np.arange(shape[k], dtype=np.float64) * fres[k] for k in range(3)]
    c = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)                               # 2. centre
    F, Wt = np.zeros(shape), np.zeros(shape)
    updated, undecided = np.zeros(shape, bool), np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            p = c @ inverse[k, :, :3].T + inverse[k, :, 3]                                 # 3. camera transform
            px, py, pz = p[..., 0], p[..., 1], p[..., 2]
            undecided |= np.abs(pz) < length_tol
            front = pz > 0
            su, sv = fx * (px / pz) + cx + 0.5, fy * (py / pz) + cy + 0.5                  # 4. projection, shifted by half a pixel
            inside = front & (su >= 0) & (su < W) & (sv >= 0) & (sv < H)                   # 4. image test
            # the image's ends are pixel boundaries too; only a voxel near an end in one coordinate and not far outside in
            # the other can go either way
            near_u, near_v = np.abs(su - np.rint(su)) < pixel_tol, np.abs(sv - np.rint(sv)) < pixel_tol
            about_u = (su > -pixel_tol) & (su < W + pixel_tol)
            about_v = (sv > -pixel_tol) & (sv < H + pixel_tol)
            undecided |= front & about_u & about_v & (near_u | near_v)
            col = np.clip(np.floor(np.where(inside, su, 0.0)), 0, W - 1).astype(np.int64)  # 5. pixel
            row = np.clip(np.floor(np.where(inside, sv, 0.0)), 0, H - 1).astype(np.int64)
            d = depth[k][row, col]
            seen = inside & (d > 0) & np.isfinite(d) & (d <= max_depth)                    # 6. depth tests: exact, the same float
            sdf = d - pz
            undecided |= seen & (np.abs(sdf + truncation) < length_tol)
            take = seen & (sdf >= -truncation)                                             # 7. band test
            f = np.minimum(sdf / truncation, 1.0)
            Wn = Wt + weight                                                               # 9. running average
            F = np.where(take, (Wt * F + weight * f) / np.where(take, Wn, 1.0), F)
            Wt = np.where(take, np.minimum(Wn, max_weight), Wt)                            # 9. weight cap
            updated |= take
    return np.stack((F, Wt), axis=-1), updated, undecided
