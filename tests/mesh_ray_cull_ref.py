"""Restatement of the culled mesh ray-casting contract (include/pvamd.h "Mesh ray casting, culled") for its tests -- TEST
INFRASTRUCTURE: mesh_ray_cull_ref.c compiled on the fly, and bounding spheres made in numpy for the tests that have no GPU to
prepare a mesh on.  The meshes and rays are those of tests/mesh_ray_ref.py."""
import ctypes
import functools
import math

import numpy as np

from pytorch_volumetric_amd import mesh_io
from tests import c_ref, mesh_ray_ref
from tests.mesh_ray_ref import Hits, _p, soup_of

TILE, GROUP = 256, 16  # PVAMD_TRI_TILE, PVAMD_TRI_GROUP


def tiles_floats(F):
    """PVAMD_TILES_FLOATS(F)"""
    return ((F + TILE - 1) // TILE) * (4 + 4 * (TILE // GROUP))


def cast(mesh, rec_of_face, tiles, origins, directions, poses=None, t_min=0.0, t_max=math.inf, normals=True, uv=True):
    """The plain loop over all triangles of `mesh` with the section's sphere_ok and point_ok, for (R, 3) rays and None or (B, 4, 4)
    poses.  rec_of_face: (F,) int32, tiles: (PVAMD_TILES_FLOATS(F),) float32 as pvamd_mesh_t documents them.  Returns
    (Hits, tests): tests (B, R) int32, the exact triangle tests made for each ray."""
    tri, nrm = soup_of(mesh)
    F = tri.shape[0]
    rec_of_face = np.ascontiguousarray(rec_of_face, np.int32).reshape(-1)
    tiles = np.ascontiguousarray(tiles, np.float32).reshape(-1)
    assert rec_of_face.shape[0] >= F and tiles.shape[0] >= tiles_floats(F)
    assert F == 0 or (np.sort(rec_of_face[:F]) == np.arange(F)).all()
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    R = o.shape[0]
    if poses is not None:
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 4, 4)
    B = 1 if poses is None else poses.shape[0]
    t = np.empty((B, R), np.float32)
    face = np.empty((B, R), np.int32)
    n_out = np.empty((B, R, 3), np.float32) if normals else None
    uv_out = np.empty((B, R, 2), np.float32) if uv else None
    tests = np.empty((B, R), np.int32)
    c_ref.load("mesh_ray_cull_ref").mesh_ray_cull_ref(
        _p(tri), _p(nrm), ctypes.c_int32(F), _p(rec_of_face), _p(tiles), _p(o), _p(d), ctypes.c_int64(R), _p(poses), ctypes.c_int32(B),
        ctypes.c_float(t_min), ctypes.c_float(t_max), _p(t), _p(face), _p(n_out), _p(uv_out), _p(tests))
    return Hits(t, face, n_out, uv_out), tests


def _enclose(centres, radii, abs_margin):
    """enclose() of csrc/mesh.hip in float32 numpy: a sphere about the mean of the records' centres, radius
    max(|c_i - mean| * 1.00001 + r_i) * 1.00001 + abs_margin."""
    f = np.float32
    mean = (centres.sum(axis=0, dtype=f) / f(len(centres))).astype(f)
    delta = centres - mean
    reach = np.sqrt((delta * delta).sum(axis=1, dtype=f)) * f(1.00001) + radii
    return np.array([mean[0], mean[1], mean[2], reach.max() * f(1.00001) + f(abs_margin)], f)


@functools.lru_cache(maxsize=None)
def _spheres_cached(mesh):
    tri = soup_of(mesh)[0]
    F = tri.shape[0]
    order = mesh_io.patch_order(tri.mean(axis=1))  # what ObjectFactory._mesh_desc hands to pvamd_mesh_prepare
    rec_of_face = np.empty(F, np.int32)
    rec_of_face[order] = np.arange(F, dtype=np.int32)
    lo, hi = mesh.aabb()
    abs_margin = 1e-6 * float(np.abs(mesh.vertices).max() + np.linalg.norm(hi - lo))
    # a record's own sphere: about the float32 centroid, through the farthest corner, rounded outwards
    centre = tri.mean(axis=1).astype(np.float32)
    far = np.linalg.norm(tri.astype(np.float64) - centre[:, None, :].astype(np.float64), axis=2).max(axis=1)
    radius = (far * 1.00001).astype(np.float32) + np.float32(abs_margin)
    centre, radius = centre[order], radius[order]
    T = (F + TILE - 1) // TILE
    tiles = np.zeros(tiles_floats(F), np.float32)
    for ti in range(T):
        a, b = ti * TILE, min(F, (ti + 1) * TILE)
        tiles[4 * ti:4 * ti + 4] = _enclose(centre[a:b], radius[a:b], abs_margin)
    for g in range((F + GROUP - 1) // GROUP):  # only groups that hold a record have a sphere
        a, b = g * GROUP, min(F, (g + 1) * GROUP)
        tiles[4 * T + 4 * g:4 * T + 4 * g + 4] = _enclose(centre[a:b], radius[a:b], abs_margin)
    rec_of_face.flags.writeable = False
    tiles.flags.writeable = False
    return rec_of_face, tiles


def standin_spheres(mesh):
    """(rec_of_face (F,) int32, tiles (PVAMD_TILES_FLOATS(F),) float32) of `mesh` without a GPU: the order is
    mesh_io.patch_order's, as in ObjectFactory._mesh_desc, and the spheres are built the way enclose() (csrc/mesh.hip) builds
    them, over records whose own sphere is a stand-in (about the centroid, not the prepared record's rectangle centre).  Every
    sphere encloses its triangles, which is all the contract asks of them.  Read-only."""
    return _spheres_cached(mesh)


# ---------------------------------------------------------------- rays: the sets of tests/test_mesh_ray_cast_gpu.py, rebuilt
H, W = 48, 64
MESHES = {"box": mesh_ray_ref.box, "field242": mesh_ray_ref.field_242, "field288": mesh_ray_ref.field_288, "drill": mesh_ray_ref.drill}


def centre_extent(name):
    lo, hi = MESHES[name]().aabb()
    return 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))


@functools.lru_cache(maxsize=None)
def image(name):
    """(origins, directions, the PLAIN loop's Hits) of the 64 x 48 pinhole image of test_pinhole_rays; read-only."""
    c, ext = centre_extent(name)
    o, d = mesh_ray_ref.pinhole(c + ext * np.array([0.9, 0.7, 1.1]), c, H, W, fov=0.6)
    want = mesh_ray_ref.cast(MESHES[name](), o, d)
    for a in (o, d, *want):
        a.flags.writeable = False
    return o, d, want


def inside_and_window_cases(name):
    """[(what, origins, directions, t_min, t_max)] of test_rays_from_inside_and_windows: rays from inside the closed mesh, windows
    that pass over the first surface, one that ends before it, one that reaches behind the origin, an empty one, and directions
    of length 0.5 and 3."""
    c, ext = centre_extent(name)
    lo, hi = MESHES[name]().aabb()
    rng = np.random.default_rng(11)
    d = rng.standard_normal((130, 3)).astype(np.float32)
    o = np.tile((lo + (hi - lo) * np.array([0.5, 0.5, 0.7])).astype(np.float32), (130, 1))
    cases = [("inside", o, d, 0.0, math.inf)]
    o, d, first = image(name)
    o, d = o[::9], d[::9]
    mid = float(np.median(first.t[0][first.face[0] >= 0]))
    cases += [("t_min", o, d, mid, math.inf), ("t_max", o, d, 0.0, mid), ("behind the origin", o, d, -10.0 * ext, mid),
              ("t_min > t_max", o, d, mid, 0.5 * mid), ("length 0.5", o, 0.5 * d, 0.0, math.inf), ("length 3", o, 3.0 * d, 0.0, math.inf)]
    return cases


def degenerate_box_rays():
    """(origins, directions) of test_degenerate_rays_on_the_box: at the vertices, along diagonals and edges, in the planes of
    faces; then six rays with a zero, NaN or infinite coordinate and a sound one."""
    V = mesh_ray_ref.box().vertices.astype(np.float32)
    o, d = [], []
    for v in V:
        for eye in (v * np.array([1, 1, 4]), v * np.array([4, 1, 1]), v * np.array([1, 4, 1]), v * 3.0, v * np.array([2, 3, 4])):
            o.append(eye)
            d.append(v - eye)
    for s in np.linspace(-1.0, 1.0, 9):
        for p in ((s, s, 5.0), (s, -s, 5.0), (s, 1.0, 5.0), (1.0, s, 5.0), (-1.0, s, 5.0)):
            o.append(p)
            d.append((0.0, 0.0, -1.0))
    for y in (-1.0, -0.5, 0.0, 0.25, 1.0):
        for z in (1.0, -1.0):
            o.append((-3.0, y, z))
            d.append((1.0, 0.0, 0.0))
        o.append((1.0, -4.0, y))
        d.append((0.0, 2.0, 0.0))
    sound = ((0.3, 0.2, 5.0), (0.0, 0.0, -1.0))
    for bad_o, bad_d in ((sound[0], (0.0, 0.0, 0.0)), (sound[0], (np.nan, 0.0, -1.0)), (sound[0], (np.nan,) * 3),
                         ((np.nan, 0.2, 5.0), sound[1]), ((0.3, np.inf, 5.0), sound[1]), (sound[0], (0.0, -np.inf, -1.0)), sound):
        o.append(bad_o)
        d.append(bad_d)
    return np.array(o, np.float32), np.array(d, np.float32)


def same_bits(a, b):
    """Hits against Hits: every bit of every output."""
    return all(x is None and y is None or np.array_equal(mesh_ray_ref.bits(x), mesh_ray_ref.bits(y)) for x, y in zip(a, b))


def assert_subset(culled, plain, what=""):
    """Every culled result is a candidate of the plain loop: where the culled mode reports a hit the plain loop reports one, with
    a t that is not larger, and with the same t the same face or a smaller id."""
    hit = culled.face >= 0
    assert (plain.face[hit] >= 0).all(), what
    assert (plain.t[hit] <= culled.t[hit]).all(), what
    tie = hit & (plain.t == culled.t)
    assert (plain.face[tie] <= culled.face[tie]).all(), what
