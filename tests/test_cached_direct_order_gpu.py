"""-m gpu: the direct cached-query kernels (csrc/cached.hip cached_query_direct) issue every gather of a lane before the
out-of-range arithmetic, run that arithmetic on ALL lanes and pick the result by a select.  What that order can get wrong --
the select, the masked gathers, the one exact-index branch shared by a lane's points, a discarded 0/0 leaking, record bits
changed on the way through -- against oracle.cached_query, bit for bit (as uint32).

Every point is placed by (tile, k, lane): lane l of the wave that owns tile t holds points t*64*PPL + 64*k + l, k < PPL.
Sizes: per direct kind the smallest point count pvamd_cached_query_kernel maps to it, and that + 191 (the last tile is then
moved back over its neighbour)."""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

# PVAMD_CQ_KERNEL_* (include/pvamd.h) of the direct kinds -> points per lane
DIRECT_PPL = {1: 1, 2: 2, 3: 2, 4: 4}
QNAN_PAYLOAD, NEG_ZERO, POS_INF, NEG_INF, DENORMAL, NEG_QNAN = 0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0xFFC00001
SPECIAL_BITS = [QNAN_PAYLOAD, NEG_ZERO, POS_INF, NEG_INF, DENORMAL, NEG_QNAN]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_smallest = {}


def smallest_size_of_kind(kind):
    """The smallest P that pvamd_cached_query_kernel maps to `kind` (scan in steps of 4096, bisect inside the step)."""
    if not _smallest:
        lib = pv._lib.load()
        k = lambda p: int(lib.pvamd_cached_query_kernel(p))
        prev = 1
        _smallest[k(1)] = 1
        for p in range(4096, (8 << 20) + 4096 + 1, 4096):
            if k(p) != k(prev):
                a, b = prev, p
                while b - a > 1:
                    m = (a + b) // 2
                    a, b = (m, b) if k(m) == k(prev) else (a, m)
                _smallest.setdefault(k(b), b)
            prev = p
    return _smallest[kind]


_caches = {}


def poisoned_cache(f64):
    """The C2-shaped drill cache with NaN (with a payload), -0.0, +-inf and a denormal written into value and gradient slots of
    a few records; returns (cache, flat indices of those records)."""
    if f64 not in _caches:
        rng = H.padded_range(H.DRILL_BB, 0.1, as_numpy=f64)
        c = pv.CachedSDF("drill_like", 0.01, rng, H.drill_like_gt(), device="cuda", cache_path=None)
        packed = c._packed.clone()
        shape = c._view.shape
        j = np.arange(24)  # records in the interior of the grid: their centres are in range whatever the rounding of the range ends
        flats = ((1 + j) * shape[1] + 2 + j) * shape[2] + 3 + j
        as_int = packed.view(torch.int32)
        for j, f in enumerate(flats):
            # every special value visits every slot (val, gx, gy, gz) over the 24 records; two slots per record
            as_int[f, j % 4] = int(np.uint32(SPECIAL_BITS[j % 6]).view(np.int32))
            as_int[f, (j + 1) % 4] = int(np.uint32(SPECIAL_BITS[(j // 4 + 3) % 6]).view(np.int32))
        c._packed = packed
        _caches[f64] = (c, flats)
    return _caches[f64]


def half_voxel_points(c, f64, n, rng):
    """In-range points on, and within a few float32 ulps of, half-voxel planes in all three coordinates (as
    test_index_fast_path_agrees_with_exact_division_at_rounding_boundaries builds them): the index estimate is unsure there."""
    v = c._view
    mn = (v.dmin if f64 else v.fmin).double().numpy()
    res = (v.dres if f64 else v.fres).double().numpy()
    k = rng.integers(0, np.array(v.shape) - 1, size=(n, 3))
    ulps = rng.integers(-6, 7, size=(n, 3))
    pts = (mn[None, :] + (k + 0.5) * res[None, :]).astype(np.float32)
    for _ in range(6):
        up, dn = np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))
        pts = np.where(ulps > 0, up, np.where(ulps < 0, dn, pts))
        ulps = ulps - np.sign(ulps)
    return pts


def build_points(c, flats, f64, P, ppl, seed):
    """(P, 3) float32 points, tile t taking pattern t mod the number of patterns.  Returns the points and a dict of index arrays
    that the test uses to check that each case really occurs."""
    rng = np.random.default_rng(seed)
    v = c._view
    rlo = np.array([float(r[0]) for r in c.ranges])
    rhi = np.array([float(r[1]) for r in c.ranges])
    bb = c.bb.cpu().double().numpy()
    T = 64 * ppl
    ntiles = P // T  # whole tiles take patterns; the ragged remainder keeps the random mix
    eps = 1e-4
    inside = rng.uniform(rlo + eps, rhi - eps, size=(P, 3)).astype(np.float32)
    in_box = rng.uniform(bb[:, 0] + eps, bb[:, 1] - eps, size=(P, 3)).astype(np.float32)
    band = in_box.copy()  # in range, outside the box: one coordinate in the padded band below the box
    ax = rng.integers(0, 3, size=P)
    band[np.arange(P), ax] = rng.uniform(rlo[ax] + eps, bb[ax, 0] - eps).astype(np.float32)
    outside = rng.uniform(rlo - 0.3, rhi + 0.3, size=(P, 3)).astype(np.float32)
    side = rng.integers(0, 2, size=P)
    outside[np.arange(P), ax] = np.where(side == 0, rlo[ax] - rng.uniform(0.001, 0.3, size=P),
                                         rhi[ax] + rng.uniform(0.001, 0.3, size=P)).astype(np.float32)
    unsure = half_voxel_points(c, f64, P, rng)
    # centres of the poisoned records, cycled
    shape = np.array(v.shape)
    fl = flats[np.arange(P) % len(flats)]
    key = np.stack([fl // (shape[1] * shape[2]), (fl // shape[2]) % shape[1], fl % shape[2]], axis=1)
    res = (v.dres if f64 else v.fres).double().numpy()
    mn = (v.dmin if f64 else v.fmin).double().numpy()
    centres = (mn[None, :] + key * res[None, :]).astype(np.float32)

    pts = np.where(rng.integers(0, 2, size=(P, 1)) == 0, inside, outside)  # the random mix, per (k, lane)
    idx = np.arange(ntiles * T)
    tile, k, lane = idx // T, (idx % T) // 64, idx % 64
    combos = 1 << ppl
    # patterns: 0 all in (inside the box), 1 all in (padded band), 2 all out, 3 alternating lanes, 4 alternating lanes flipped per k,
    # 5 .. 5+combos-1: point k in range iff bit k of the combination, 5+combos: poisoned records in even lanes,
    # +1 .. +5: one unsure point at (k0, l0), the lane's other points NaN / +inf / -inf / far out / in range, the rest random,
    # +6: one unsure point alone in a wave of out-of-range points
    n_pat = 5 + combos + 1 + 5 + 1
    pat = tile % n_pat
    pts_t = pts[:ntiles * T].copy()

    def put(mask, src):
        pts_t[mask] = src[:ntiles * T][mask]

    put(pat == 0, in_box)
    put(pat == 1, band)
    put(pat == 2, outside)
    alt = lane % 2 == 0
    put((pat == 3) & alt, inside); put((pat == 3) & ~alt, outside)
    alt_k = (lane + k) % 2 == 0
    put((pat == 4) & alt_k, inside); put((pat == 4) & ~alt_k, outside)
    for combo in range(combos):
        m = pat == 5 + combo
        k_in = ((combo >> k) & 1) == 1
        put(m & k_in, inside)
        put(m & ~k_in, outside)
    rec_pat = 5 + combos
    put((pat == rec_pat) & alt, centres); put((pat == rec_pat) & ~alt, outside)
    k0, l0 = (tile // n_pat) % ppl, (tile * 7) % 64  # the slot moves over every k and lane
    at_slot = (k == k0) & (lane == l0)
    same_lane_other_k = (k != k0) & (lane == l0)
    for j in range(5):
        m = pat == rec_pat + 1 + j
        put(m & at_slot, unsure)
        if j == 0:
            pts_t[m & same_lane_other_k] = np.float32(np.nan)
        elif j == 1:
            pts_t[m & same_lane_other_k] = np.float32(np.inf)
        elif j == 2:
            pts_t[m & same_lane_other_k] = np.float32(-np.inf)
        elif j == 3:
            pts_t[m & same_lane_other_k] = np.float32(1e30)
        else:
            put(m & same_lane_other_k, inside)
    alone = pat == rec_pat + 6
    put(alone, outside); put(alone & at_slot, unsure)
    pts[:ntiles * T] = pts_t
    where = {"in_box": idx[pat == 0], "band": idx[pat == 1], "records": idx[(pat == rec_pat) & alt],
             "unsure": idx[(pat > rec_pat) & at_slot], "alone": idx[alone & at_slot], "alone_rest": idx[alone & ~at_slot],
             "all_out": idx[pat == 2], "n_pat": n_pat}
    return np.ascontiguousarray(pts), where


@pytest.mark.parametrize("ragged", [0, 191])
@pytest.mark.parametrize("kind", sorted(DIRECT_PPL))
@pytest.mark.parametrize("f64", [True, False])
def test_direct_kernel_lane_patterns_records_and_both_oob_modes_bitwise(f64, kind, ragged):
    lib = pv._lib.load()
    ppl = DIRECT_PPL[kind]
    P = smallest_size_of_kind(kind) + ragged
    assert int(lib.pvamd_cached_query_kernel(P)) == kind
    if kind == 1:
        assert smallest_size_of_kind(kind) == 16384
    c, flats = poisoned_cache(f64)
    pts_np, where = build_points(c, flats, f64, P, ppl, seed=1000 * kind + ragged + (7 if f64 else 0))
    assert P // (64 * ppl) >= 2 * where["n_pat"]  # every pattern fills several whole waves
    pts = torch.from_numpy(pts_np).cuda()
    vbuf = torch.empty(P + 3, device="cuda")
    gbuf = torch.empty(3 * P + 5, device="cuda")
    obuf = torch.empty(P + 2, dtype=torch.uint8, device="cuda")
    val, grad, mask = vbuf[1:1 + P], gbuf[1:1 + 3 * P], obuf[1:1 + P]  # a sentinel either side of every output
    packed_bits = c._packed.cpu().numpy().view(np.uint32)
    for mode in (pv.OutOfBoundsStrategy.BOUNDING_BOX, pv.OutOfBoundsStrategy.LOOKUP_GT_SDF):
        bbox = mode == pv.OutOfBoundsStrategy.BOUNDING_BOX
        og = H.oracle_grid_from_cached(c, oob_mode=1 if bbox else 0)
        oval, ograd, ooob = oracle.cached_query(og, pts_np)
        # the cases are really there
        assert not ooob[where["in_box"]].any() and not ooob[where["band"]].any() and not ooob[where["records"]].any()
        assert ooob[where["all_out"]].all() and ooob[where["alone_rest"]].all()
        assert not ooob[where["unsure"]].any() and len(where["alone"]) > 0 and len(where["unsure"]) > len(where["alone"])
        got_special = set(_bits(oval[where["records"]]).tolist()) | set(_bits(ograd[where["records"]]).ravel().tolist())
        assert set(SPECIAL_BITS) <= got_special  # gathered by some lanes, and the oracle hands them on as stored
        if bbox:  # the discarded bounding-box value: 0/0 inside the box, finite in the padded band
            bb = c.bb.cpu().float().numpy()
            q_box, q_band = pts_np[where["in_box"]], pts_np[where["band"]]
            assert ((q_box >= bb[:, 0]) & (q_box <= bb[:, 1])).all()
            assert (np.maximum(bb[:, 0] - q_band, q_band - bb[:, 1]).max(axis=1) > 0).all()
        else:  # LOOKUP_GT_SDF: out-of-range lanes give zeros
            assert not _bits(oval[ooob]).any() and not _bits(ograd[ooob]).any()
        desc = c._grid_desc(oob_mode=mode)
        for want_mask in (True, False):
            vbuf.fill_(-7.0); gbuf.fill_(-7.0); obuf.fill_(9)
            pv._lib.check(lib.pvamd_cached_query(ctypes.byref(desc), pv._lib.ptr(pts), P, pv._lib.ptr(val), pv._lib.ptr(grad),
                                                 pv._lib.ptr(mask) if want_mask else None, pv._lib.stream_ptr()),
                          "pvamd_cached_query")
            torch.cuda.synchronize()
            tag = (P, bbox, want_mask)
            gv, gg = _bits(val.cpu().numpy()), _bits(grad.cpu().numpy()).reshape(P, 3)
            bad = np.nonzero((gv != _bits(oval)) | (gg != _bits(ograd)).any(axis=1))[0]
            assert bad.size == 0, (tag, bad[:8], pts_np[bad[:8]])
            # in-range lanes return the stored record, bit for bit (NaN payloads, -0, inf and denormals included)
            inb = np.nonzero(~ooob)[0]
            okey, oflat, _ = oracle.voxel_index(og, pts_np[inb])
            assert np.array_equal(gv[inb], packed_bits[oflat, 0]) and np.array_equal(gg[inb], packed_bits[oflat, 1:4]), tag
            assert float(vbuf[0]) == -7.0 and float(vbuf[1 + P]) == -7.0 and float(gbuf[0]) == -7.0 and float(gbuf[1 + 3 * P]) == -7.0, tag
            if want_mask:
                assert np.array_equal(mask.cpu().numpy().astype(bool), ooob), tag
                assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0, 1}, tag
                assert int(obuf[0]) == 9 and int(obuf[1 + P]) == 9, tag
            else:
                assert (obuf == 9).all(), tag
