"""Restatement of the mesh ray-casting contract (include/pvamd.h "Mesh ray casting") for its tests -- TEST INFRASTRUCTURE:
mesh_ray_ref.c compiled on the fly, and the meshes and rays the CPU and GPU tests share."""
import ctypes
import functools
import math
from typing import NamedTuple

import numpy as np

from pytorch_volumetric_amd import mesh_io
from tests import c_ref
from tests.tsdf_ref import look_at


class Hits(NamedTuple):
    t: np.ndarray        # (B, R) float32, +inf on a miss
    face: np.ndarray     # (B, R) int32, -1 on a miss
    normal: np.ndarray   # (B, R, 3) float32, None when not asked for
    uv: np.ndarray       # (B, R, 2) float32, None when not asked for


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def soup_of(mesh):
    """((F, 3, 3) float32 corners, (F, 3) float32 normals) of a mesh_io.TriMesh, in original face order: what an ObjectFactory
    uploads (sdf.py _mesh_desc), before its spatial sort."""
    return (np.ascontiguousarray(mesh.triangle_soup().astype(np.float32)),
            np.ascontiguousarray(mesh.triangle_normals().astype(np.float32)))


def cast(mesh, origins, directions, poses=None, t_min=0.0, t_max=math.inf, normals=True, uv=True):
    """The plain loop over all triangles of `mesh` for (R, 3) rays and None or (B, 4, 4) poses."""
    tri, nrm = soup_of(mesh)
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
    c_ref.load("mesh_ray_ref").mesh_ray_ref(_p(tri), _p(nrm), ctypes.c_int32(tri.shape[0]), _p(o), _p(d), ctypes.c_int64(R), _p(poses),
                                            ctypes.c_int32(B), ctypes.c_float(t_min), ctypes.c_float(t_max), _p(t), _p(face), _p(n_out),
                                            _p(uv_out))
    return Hits(t, face, n_out, uv_out)


def assert_same(got, want, what=""):
    """A MeshRayHits of float32 tensors against the restatement's Hits: every bit of every output."""
    pairs = [("t", got.t, want.t), ("face", got.face_ids, want.face)]
    if want.normal is not None:
        pairs.append(("normal", got.normals, want.normal))
    if want.uv is not None:
        pairs.append(("uv", got.uv, want.uv))
    for name, g, w in pairs:
        g = g.cpu().numpy()
        if name == "face":
            g = g.astype(np.int32)
        g = g.reshape(w.shape)
        assert g.dtype == w.dtype, (what, name, g.dtype)
        differ = bits(g) != bits(w)
        assert not differ.any(), (what, name, int(differ.sum()), np.argwhere(differ)[:4].tolist())


# ---------------------------------------------------------------- meshes
@functools.lru_cache(maxsize=None)
def box():
    """The 12-triangle box template of tests/golden/meshes: one partial group."""
    from tests import helpers
    return mesh_io.load_mesh(helpers.mesh_path("box_template.obj"))


@functools.lru_cache(maxsize=None)
def height_field(nx, ny, seed=5):
    """A bumpy open sheet over [-1, 1]^2 of (nx - 1) * (ny - 1) * 2 triangles whose normals point to +z on the whole: height
    0.15 * (sin, cos) waves plus seeded noise, so that no two triangles are coplanar."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-1.0, 1.0, nx), np.linspace(-1.0, 1.0, ny), indexing="ij")
    z = 0.15 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y - 0.2) + 0.02 * rng.standard_normal(x.shape)
    vertices = np.stack((x, y, z), axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    v00, v10, v01, v11 = i * ny + j, (i + 1) * ny + j, i * ny + j + 1, (i + 1) * ny + j + 1
    faces = np.stack((np.stack((v00, v10, v11), -1), np.stack((v00, v11, v01), -1)), axis=-2).reshape(-1, 3)
    return mesh_io.TriMesh(vertices, faces)


def field_242():
    """242 triangles: one tile whose last group holds 2 records."""
    return height_field(12, 12)


def field_288():
    """288 triangles: two tiles, the second with 32 records and the rest padding."""
    return height_field(13, 13)


@functools.lru_cache(maxsize=None)
def drill():
    from tests import helpers
    return mesh_io.load_mesh(helpers.mesh_path("ycb_power_drill.npz"))


# ---------------------------------------------------------------- rays
def pinhole(eye, target, height, width, fov=0.9):
    """(origins, directions) (height * width, 3) float32 of pv.camera_rays for a camera at `eye` looking at `target` whose image
    spans about `fov` radians across its width."""
    import torch
    import pytorch_volumetric_amd as pv
    f = 0.5 * width / math.tan(0.5 * fov)
    pose = torch.from_numpy(look_at(eye, target)).to(torch.float32)
    o, d = pv.camera_rays((f, f, 0.5 * (width - 1), 0.5 * (height - 1)), height, width, pose)
    return np.ascontiguousarray(o.expand_as(d).reshape(-1, 3).numpy()), np.ascontiguousarray(d.reshape(-1, 3).numpy())


def extent(mesh):
    lo, hi = mesh.aabb()
    return float(np.linalg.norm(hi - lo))


def rigid(seed, shift=0.3, about=(0.0, 0.0, 0.0)):
    """A (4, 4) float32 rigid matrix: a random rotation about the point `about` and a translation of up to `shift`."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    about = np.asarray(about, np.float64)
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, about - q @ about + rng.uniform(-shift, shift, 3)
    return m.astype(np.float32)


IN_PLANE_SEEDS = (101, 102, 105)  # rotations for which in_plane_rays(seed, 30000) holds noise hits of both kinds


@functools.lru_cache(maxsize=None)
def rotated_box(seed):
    """The box template turned into general position by rigid(seed)'s rotation: its arithmetic rounds."""
    R = rigid(seed, 0.0).astype(np.float64)[:3, :3]
    return mesh_io.TriMesh(box().vertices @ R.T, box().faces)


def in_plane_rays(seed, n):
    """(origins, directions (n, 3) float32, away (n,), beside (n,)) for rotated_box(seed): rays that lie, up to the rounding of
    the rotation, in the plane of the box's top face, from 3 to 50 units off its centre.  `away`: the ray points away from
    the face and every corner of the box is behind its origin.  `beside`: its line passes more than 3 units from the box's
    centre, whose corners are 1.74 from it.  For such rays den, U, V and T of the face's two triangles are all rounding noise."""
    R = rigid(seed, 0.0).astype(np.float64)[:3, :3]
    rng = np.random.default_rng(seed)
    ang, rho = rng.uniform(0, 2 * np.pi, n), rng.uniform(3.0, 50.0, n)
    o = np.stack((rho * np.cos(ang), rho * np.sin(ang), np.ones(n)), -1)
    turn = ang + rng.uniform(-1.4, 1.4, n)
    d = np.stack((np.cos(turn), np.sin(turn), np.zeros(n)), -1)
    beside = np.abs(o[:, 0] * d[:, 1] - o[:, 1] * d[:, 0]) > 3.0
    away = ((box().vertices[None, :, :] - o[:, None, :]) * d[:, None, :]).sum(-1).max(axis=1) < -1.0
    return (o @ R.T).astype(np.float32), (d @ R.T).astype(np.float32), away, beside


# ---------------------------------------------------------------- an independent float64 formulation
def moller_trumbore(mesh, origins, directions, t_min=0.0, t_max=math.inf):
    """Textbook Moeller-Trumbore in float64 over the float32 soup: edge vectors from corner a, p = d x e2, det = e1 . p,
    u = (s . p) / det, q = s x e1, v = (d . q) / det, t = (e2 . q) / det.  Returns per ray (t (R,), face (R,) -1 on a miss,
    margin (R,)): margin is the smallest distance of a barycentric from 0 (or of their sum from 1) over the triangles whose plane
    the ray crosses in or next to the triangle, and 0 when some triangle's det is not sound (|det| < 1e-6 |n| |d|): rays with a
    small margin are the ones a float32 evaluation may decide differently."""
    tri = soup_of(mesh)[0].astype(np.float64)
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.cross(e1, e2)
    p = np.cross(d[:, None, :], e2[None, :, :])                 # (R, F, 3)
    det = np.einsum("fk,rfk->rf", e1, p)
    s = o[:, None, :] - a[None, :, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.einsum("rfk,rfk->rf", s, p) / det
        q = np.cross(s, e1[None, :, :])
        v = np.einsum("rk,rfk->rf", d, q) / det
        t = np.einsum("fk,rfk->rf", e2, q) / det
    sound = np.abs(det) >= 1e-6 * np.linalg.norm(n, axis=1)[None, :] * np.linalg.norm(d, axis=1)[:, None]
    inside = sound & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= t_min) & (t <= t_max)
    tt = np.where(inside, t, np.inf)
    face = np.where(inside.any(axis=1), tt.argmin(axis=1), -1)
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1.0 - u - v))
        almost = (u >= -1e-3) & (v >= -1e-3) & (u + v <= 1.0 + 1e-3)  # elsewhere an edge's LINE is close, not the edge
    margin = np.where(sound, np.where(almost, edge, np.inf), 0.0).min(axis=1)
    return tt.min(axis=1), face, margin
