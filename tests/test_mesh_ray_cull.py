"""Culled mesh ray casting without a GPU: the restatement of include/pvamd.h "Mesh ray casting, culled"
(tests/mesh_ray_cull_ref.c) against the plain loop (tests/mesh_ray_ref.c) -- a subset of its candidates everywhere, its bits on
generic rays, and next to none of the rounding-noise hits of rays in a face's plane -- with bounding spheres made in numpy the
way enclose() (csrc/mesh.hip) makes them; and the argument errors, the header section and its binding."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import mesh_ray_cull_ref as C
from tests import mesh_ray_ref as M


def both(mesh, o, d, poses=None, t_min=0.0, t_max=math.inf, plain=None):
    rec_of_face, tiles = C.standin_spheres(mesh)
    culled, tests = C.cast(mesh, rec_of_face, tiles, o, d, poses, t_min, t_max)
    plain = plain if plain is not None else M.cast(mesh, o, d, poses, t_min, t_max)
    C.assert_subset(culled, plain)
    assert (tests >= 0).all() and (tests <= mesh.faces.shape[0]).all()
    return culled, plain, tests


def test_standin_spheres_enclose_their_triangles():
    """Every corner of every triangle lies inside the sphere of its tile and of its group, in float64; groups that begin at or
    past F have no sphere."""
    for name in C.MESHES:
        mesh = C.MESHES[name]()
        tri = M.soup_of(mesh)[0].astype(np.float64)
        F = tri.shape[0]
        rec_of_face, tiles = C.standin_spheres(mesh)
        T = (F + 255) // 256
        assert tiles.shape == (C.tiles_floats(F),) and tiles.shape[0] == 68 * T
        tile = tiles[:4 * T].reshape(T, 4).astype(np.float64)[rec_of_face // 256]
        group = tiles[4 * T:].reshape(16 * T, 4).astype(np.float64)[rec_of_face // 16]
        for s in (tile, group):
            assert (np.linalg.norm(tri - s[:, None, :3], axis=2).max(axis=1) < s[:, 3]).all(), name
        assert not tiles[4 * T + 4 * ((F + 15) // 16):].any()


@pytest.mark.parametrize("name", list(C.MESHES))
def test_images_keep_the_plain_bits(name):
    """The 64 x 48 image of each mesh: the culled mode reports the plain loop's bits on every ray, and makes a fraction of its
    exact tests."""
    o, d, plain = C.image(name)
    mesh = C.MESHES[name]()
    culled, _, tests = both(mesh, o, d, plain=plain)
    assert 0.15 < (plain.face[0] >= 0).mean() < 0.95
    assert C.same_bits(culled, plain)
    hit = plain.face[0] >= 0
    assert (tests[0][hit] >= 1).all()
    if name == "drill":
        assert tests.mean() < 0.02 * mesh.faces.shape[0]


@pytest.mark.parametrize("name", ["box", "drill"])
def test_inside_and_window_rays_keep_the_plain_bits(name):
    mesh = C.MESHES[name]()
    for what, o, d, t_min, t_max in C.inside_and_window_cases(name):
        culled, plain, tests = both(mesh, o, d, t_min=t_min, t_max=t_max)
        assert C.same_bits(culled, plain), what
        if what == "inside":
            assert (culled.face >= 0).all()
        if what == "t_min > t_max":
            assert (culled.face == -1).all() and not tests.any()  # inf * 0 aside, no sphere passes an empty window
        if what == "t_max":
            assert (plain.face >= 0).any() and (plain.face < 0).any()


def test_degenerate_box_rays_keep_the_plain_bits():
    """Rays at vertices, along edges and diagonals and in the planes of faces of the axis-aligned box, whose arithmetic is exact;
    a ray with a NaN or infinite coordinate or a zero direction passes no sphere test at all."""
    o, d = C.degenerate_box_rays()
    poses = np.stack([M.rigid(3), np.eye(4, dtype=np.float32)])
    for p in (None, poses):
        culled, plain, tests = both(M.box(), o, d, poses=p)
        assert C.same_bits(culled, plain)
        assert (culled.face[:, -7:-1] == -1).all() and (culled.face[:, -1] >= 0).all() and not tests[:, -7:-1].any()
        assert (culled.face[-1][:40] >= 0).all()  # unposed, or the identity: every ray at a vertex hits


@pytest.mark.parametrize("seed", M.IN_PLANE_SEEDS)
def test_rays_in_a_rounded_plane_lose_their_noise_hits(seed):
    """Rays that lie, up to rounding, in the plane of a face of a rotated box.  The plain loop keeps hits for rays that point away
    from the box and for lines that pass 3 units beside it; the culled mode keeps a hit only where the point o + t d lies in the
    box's tile sphere, and what it keeps has the plain loop's bits.
    point_ok is what this rests on: sphere_ok alone keeps one hit of seed 101 whose line meets the sphere and whose point lies
    3.877 from the centre of a tile sphere of radius 2.596."""
    o, d, away, beside = M.in_plane_rays(seed, 30000)
    mesh = M.rotated_box(seed)
    culled, plain, _ = both(mesh, o, d)
    hit = plain.face[0] >= 0
    assert (hit & away).sum() >= 5 and (hit & beside).sum() >= 5
    kept = culled.face[0] >= 0
    for a, b in zip(culled, plain):
        assert np.array_equal(M.bits(a[0][kept]), M.bits(b[0][kept]))
    sphere = C.standin_spheres(mesh)[1][:4].astype(np.float64)
    point = o[kept].astype(np.float64) + culled.t[0][kept].astype(np.float64)[:, None] * d[kept].astype(np.float64)
    print("seed", seed, "plain hits", int(hit.sum()), "away", int((hit & away).sum()), "beside", int((hit & beside).sum()),
          "culled hits", int(kept.sum()), "at", np.linalg.norm(point - sphere[:3], axis=1).tolist(), "of", float(sphere[3]))
    assert (np.linalg.norm(point - sphere[:3], axis=1) <= sphere[3]).all()


def test_slack_of_the_sphere_test():
    """The constant 4e-7 of rs against the bound the header states for it: q and wd evaluated in float32 are within
    4 * 2^-24 |w| |d| of their float64 values, for far origins and long and short directions."""
    rng = np.random.default_rng(3)
    n = 20000
    w = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-2, 4, (n, 1))).astype(np.float32)
    d = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    f = np.float32
    q32 = np.stack([w[:, 1] * d[:, 2] - w[:, 2] * d[:, 1], w[:, 2] * d[:, 0] - w[:, 0] * d[:, 2], w[:, 0] * d[:, 1] - w[:, 1] * d[:, 0]], -1)
    assert q32.dtype == f  # every product and difference rounded on its own: no better than the contract's fmaf
    wd32 = (w[:, 2] * d[:, 2] + (w[:, 1] * d[:, 1] + w[:, 0] * d[:, 0])).astype(f)
    w64, d64 = w.astype(np.float64), d.astype(np.float64)
    scale = np.linalg.norm(w64, axis=1) * np.linalg.norm(d64, axis=1)
    bound = 4.0 * 2.0 ** -24 * scale
    assert (np.linalg.norm(q32.astype(np.float64) - np.cross(w64, d64), axis=1) <= bound).all()
    assert (np.abs(wd32.astype(np.float64) - (w64 * d64).sum(-1)) <= bound).all()
    assert 4.0 * 2.0 ** -24 < 4e-7


# ---------------------------------------------------------------- argument errors, with no GPU
def test_cull_must_be_a_bool():
    obj = pv.MeshObjectFactory(mesh=M.box())
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    for bad in (1, 0, None, "True", 1.0, np.True_):
        with pytest.raises(TypeError):
            obj.cast_rays(o, d, cull=bad)
        with pytest.raises(TypeError):
            obj.render_depth((70.0, 65.0, 31.5, 22.0), 4, 4, torch.eye(4), cull=bad)
    with pytest.raises(ValueError):  # the other checks still come before a GPU is asked for
        obj.cast_rays(torch.zeros(5, 2), d, cull=True)


def test_entry_point_argument_errors():
    """The codes of pvamd_mesh_ray_cast_culled that return before any launch: those of pvamd_mesh_ray_cast, and PVAMD_E_NULL for
    faces without `tiles`."""
    lib = _lib.load()
    desc = _lib.MeshDesc()
    inf = math.inf

    def call(mesh, R, poses, B, t_min=0.0, t_max=inf, rays=1, out=1):
        return lib.pvamd_mesh_ray_cast_culled(ctypes.byref(mesh) if mesh is not None else None, rays, rays, R, poses, B, t_min, t_max, out,
                                              out, None, None, None)

    assert call(desc, -1, None, 1) == _lib.E_SHAPE and call(desc, 4, None, 2) == _lib.E_SHAPE and call(desc, 4, 16, -1) == _lib.E_SHAPE
    assert call(desc, 2 ** 31, None, 1) == _lib.E_SHAPE and call(desc, 2 ** 16, 16, 2 ** 15) == _lib.E_SHAPE
    assert call(None, 4, None, 1) == _lib.H["PVAMD_E_NULL"]
    assert call(desc, 4, None, 1, t_min=math.nan) == _lib.H["PVAMD_E_MODE"] and call(desc, 4, None, 1, t_max=math.nan) == _lib.H["PVAMD_E_MODE"]
    assert call(desc, 0, None, 1) == 0 and call(desc, 4, 16, 0) == 0  # nothing to do: nothing is launched
    assert call(desc, 4, None, 1, rays=None) == _lib.H["PVAMD_E_NULL"] and call(desc, 4, None, 1, out=None) == _lib.H["PVAMD_E_NULL"]
    desc.F = 3
    assert call(desc, 4, None, 1) == _lib.H["PVAMD_E_NULL"]  # faces and no records
    desc.rec = 4096
    assert call(desc, 4, None, 1) == _lib.H["PVAMD_E_NULL"]  # records and no tile spheres
    desc.rec, desc.tiles = 4100, 4096
    assert call(desc, 4, None, 1) == _lib.H["PVAMD_E_ALIGN"]
    desc.F = -1
    assert call(desc, 4, None, 1) == _lib.E_SHAPE


def test_header_section_and_binding():
    assert _lib.ABI_VERSION == 16 and _lib.load().pvamd_abi_version() == 16  # an additive entry point
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvamd.h")) as f:
        text = f.read()
    assert "---- Mesh ray casting, culled" in text and "fmaf(4e-7f, sqrt(ww), r * 1.00001f)" in text
    assert _lib.SIGNATURES["pvamd_mesh_ray_cast_culled"] == _lib.SIGNATURES["pvamd_mesh_ray_cast"]
    assert hasattr(_lib.load(), "pvamd_mesh_ray_cast_culled")
