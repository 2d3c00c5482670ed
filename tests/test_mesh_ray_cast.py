"""Mesh ray casting without a GPU: the restatement (tests/mesh_ray_ref.c) against an independent float64 formulation, the uv
convention, camera_rays against the TSDF projection, the argument errors, and the header section and its binding."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import mesh_ray_ref as M
from tests import tsdf_ref

# three eyes in general position: no ray is parallel to a face of the box or runs along an edge of the sheet
EYES = ((2.9, 2.1, 3.3), (-3.2, 1.7, 2.4), (0.8, -3.4, 2.7))
H, W = 24, 32


def rays_from_eyes():
    parts = [M.pinhole(eye, (0.03, -0.02, 0.01), H, W, fov=0.75) for eye in EYES]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("mesh", [M.box, lambda: M.height_field(9, 11)], ids=["box", "height_field"])
def test_restatement_against_float64(mesh):
    """Hit or miss and the face agree and t agrees to 1e-5 relative, on the rays the float64 formulation decides soundly: its
    barycentrics at least 1e-4 from an edge and every |det| at least 1e-6 |n| |d|.  At most 5 % of the rays are left out."""
    mesh = mesh()
    o, d = rays_from_eyes()
    want_t, want_face, margin = M.moller_trumbore(mesh, o, d)
    keep = margin >= 1e-4
    assert (~keep).mean() <= 0.05, (~keep).mean()
    got = M.cast(mesh, o, d)
    t, face = got.t[0], got.face[0]
    assert (want_face[keep] >= 0).mean() > 0.2 and (want_face[keep] < 0).any()  # the images show the mesh and its surroundings
    assert np.array_equal(face[keep], want_face[keep])
    hit = keep & (want_face >= 0)
    assert np.all(np.abs(t[hit].astype(np.float64) - want_t[hit]) <= 1e-5 * np.abs(want_t[hit]))
    assert np.all(np.isposinf(t[face < 0])) and not got.normal[0][face < 0].any() and not got.uv[0][face < 0].any()
    # the normal is the stored one, as it is
    nrm = M.soup_of(mesh)[1]
    assert np.array_equal(got.normal[0][face >= 0], nrm[face[face >= 0]] + np.float32(0))


@pytest.mark.parametrize("mesh", [M.box, M.field_242], ids=["box", "height_field"])
def test_uv_weights_corners_b_and_c(mesh):
    """(1 - u - v) a + u b + v c reproduces o + t d to 1e-5 of the mesh's extent."""
    mesh = mesh()
    o, d = rays_from_eyes()
    got = M.cast(mesh, o, d)
    hit = got.face[0] >= 0
    assert hit.sum() > 100
    tri = M.soup_of(mesh)[0].astype(np.float64)[got.face[0][hit]]
    u, v = got.uv[0][hit, 0].astype(np.float64)[:, None], got.uv[0][hit, 1].astype(np.float64)[:, None]
    from_uv = (1.0 - u - v) * tri[:, 0] + u * tri[:, 1] + v * tri[:, 2]
    along = o[hit].astype(np.float64) + got.t[0][hit].astype(np.float64)[:, None] * d[hit].astype(np.float64)
    assert np.abs(from_uv - along).max() <= 1e-5 * M.extent(mesh)
    assert (u > 0.05).any() and (v > 0.05).any()  # not a test of corner a alone


def test_restatement_rules():
    """Ties go to the smallest face id, the window passes over the first surface, t scales with 1 / |d|, poses agree with moved
    rays, and the identity pose gives the bits of no pose."""
    box = M.box()
    faces = box.faces
    top = [f for f in range(12) if (box.vertices[faces[f]][:, 2] == 1.0).all()]
    assert len(top) == 2
    shared = set(faces[top[0]]) & set(faces[top[1]])  # the diagonal of the top face
    p, q = (box.vertices[i] for i in shared)
    o = np.array([[0.25 * p[0] + 0.75 * q[0], 0.25 * p[1] + 0.75 * q[1], 5.0], [p[0], p[1], 5.0], [0.3, 0.2, 5.0], [0.3, 0.2, 0.0]], np.float32)
    d = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (4, 1))
    got = M.cast(box, o, d)
    assert got.face[0, 0] == min(top) and got.t[0, 0] == 4.0                  # on the diagonal: two candidates, equal t
    assert got.face[0, 1] == min(top)                                         # at a corner both of them share; the side faces have den = 0
    assert got.t[0, 1] == 4.0 and got.t[0, 2] == 4.0 and got.t[0, 3] == 1.0   # the last one starts inside and leaves through the bottom
    second = M.cast(box, o[2:3], d[2:3], t_min=4.5)
    assert second.t[0, 0] == 6.0 and (box.vertices[faces[second.face[0, 0]]][:, 2] == -1.0).all()
    assert M.cast(box, o[2:3], d[2:3], t_max=3.5).face[0, 0] == -1
    assert M.cast(box, o[2:3], d[2:3], t_min=2.0, t_max=1.0).face[0, 0] == -1
    assert M.cast(box, o[2:3], 0.5 * d[2:3]).t[0, 0] == 8.0 and M.cast(box, o[2:3], 4.0 * d[2:3]).t[0, 0] == 1.0
    assert M.cast(box, o[2:3], -d[2:3], t_min=-10.0).t[0, 0] == -6.0           # a negative window looks behind the origin
    for bad in (np.zeros(3), [np.nan, 0, -1]):
        miss = M.cast(box, o[2:3], np.array([bad], np.float32))
        assert miss.face[0, 0] == -1 and np.isposinf(miss.t[0, 0])
    in_plane = M.cast(box, np.array([[-3.0, 0.1, 1.0]], np.float32), np.array([[1.0, 0.0, 0.0]], np.float32))
    assert in_plane.face[0, 0] not in top                                      # den = 0 drops the two triangles it lies in
    # poses: a rigid world_to_object applied by the restatement against rays moved in float64
    oo, dd = rays_from_eyes()
    oo, dd = oo[::7], dd[::7]
    poses = np.stack([np.eye(4, dtype=np.float32), M.rigid(1), M.rigid(2)])
    posed = M.cast(box, oo, dd, poses)
    plain = M.cast(box, oo, dd)
    for name in ("t", "face", "normal", "uv"):
        assert np.array_equal(M.bits(getattr(posed, name)[0]), M.bits(getattr(plain, name)[0])), name
    for b in (1, 2):
        R, tr = poses[b, :3, :3].astype(np.float64), poses[b, :3, 3].astype(np.float64)
        moved = M.cast(box, oo @ R.T + tr, dd @ R.T)
        same = (moved.face[0] == posed.face[b]) & (moved.face[0] >= 0)
        assert same.mean() > 0.2 and (moved.face[0] != posed.face[b]).mean() < 0.02
        assert np.allclose(moved.t[0][same], posed.t[b][same], rtol=1e-4)
        assert np.allclose(moved.normal[0][same] @ R, posed.normal[b][same], atol=1e-5)  # R^T n, row by row


@pytest.mark.parametrize("seed", M.IN_PLANE_SEEDS)
def test_rays_in_a_rounded_plane_hit_wherever_the_line_runs(seed):
    """What the contract's float32 test does with a ray that lies, up to rounding, in a triangle's plane: den, U, V and T are
    noise, and the plain loop reports candidates with a positive finite t for triangles wholly behind the origin and for lines
    that pass well beside the mesh.  This is why the kernel culls nothing; the float64 formulation reports none of them."""
    o, d, away, beside = M.in_plane_rays(seed, 30000)
    got = M.cast(M.rotated_box(seed), o, d, normals=False, uv=False)
    hit = got.face[0] >= 0
    assert (hit & away).sum() >= 5 and (hit & beside).sum() >= 5
    assert (got.t[0][hit & away] > 0).all() and np.isfinite(got.t[0][hit & away]).all()
    pick = np.flatnonzero(hit & (away | beside))[:50]
    _, face64, _ = M.moller_trumbore(M.rotated_box(seed), o[pick], d[pick])
    assert (face64 == -1).all()


# ---------------------------------------------------------------- camera_rays
INTRINSICS = (70.0, 65.0, 31.5, 22.0)


def test_camera_rays_shapes_and_errors():
    o, d = pv.camera_rays(INTRINSICS, 48, 64)
    assert o.shape == (1, 1, 3) and d.shape == (48, 64, 3) and d.dtype == torch.float32 and not o.any()
    assert torch.allclose(d.norm(dim=-1), torch.ones(48, 64), atol=1e-6)
    assert torch.equal(d[22, :, 1], torch.zeros(64)) and d[0, 0, 0] < 0 and d[0, 0, 1] < 0 and (d[..., 2] > 0).all()  # x right, y down
    K3 = [[70.0, 0, 31.5], [0, 65.0, 22.0], [0, 0, 1]]
    assert torch.equal(pv.camera_rays(K3, 48, 64)[1], d)
    poses = torch.from_numpy(tsdf_ref.axis_views((0.1, 0.2, 0.3), 2.0)).to(torch.float32)
    o, dk = pv.camera_rays(INTRINSICS, 48, 64, poses)
    assert o.shape == (6, 1, 1, 3) and dk.shape == (6, 48, 64, 3) and torch.equal(o[:, 0, 0], poses[:, :3, 3])
    assert torch.equal(pv.camera_rays(INTRINSICS, 48, 64, poses[2])[1], dk[2])
    assert torch.allclose(dk[3], d @ poses[3, :3, :3].T, atol=1e-6)
    assert pv.camera_rays(INTRINSICS, 48, 64, poses.double())[1].dtype == torch.float64
    with pytest.raises(ValueError):
        pv.camera_rays((70.0, 65.0, 31.5), 48, 64)
    with pytest.raises(ValueError):
        pv.camera_rays(INTRINSICS, 0, 64)
    with pytest.raises(ValueError):
        pv.camera_rays(INTRINSICS, 48, 64, torch.eye(3))


def test_camera_rays_match_the_tsdf_projection():
    """A point on a pixel's ray, projected by statements 3 to 5 of "TSDF integration" as tests/tsdf_ref.c spells them, lands on
    that pixel."""
    Hh, Ww = 48, 64
    fx, fy, cx, cy = (np.float32(v) for v in INTRINSICS)
    for pose in tsdf_ref.wall_frames(((-1, 1), (-1, 1), (-1, 1)), 0.25)[1]:
        o, d = pv.camera_rays(INTRINSICS, Hh, Ww, torch.from_numpy(np.array(pose)).to(torch.float32))
        T = tsdf_ref.invert(pose[None])[0]
        for depth in (0.7, 3.1):
            c = (o + np.float32(depth) * d).numpy().astype(np.float32)
            px, py, pz = (((T[i, 0] * c[..., 0] + T[i, 1] * c[..., 1]) + T[i, 2] * c[..., 2]) + T[i, 3] for i in range(3))
            u, v = fx * (px / pz) + cx, fy * (py / pz) + cy
            rows, cols = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
            assert (pz > 0).all()
            assert np.array_equal(np.floor(u + np.float32(0.5)).astype(np.int64), cols)
            assert np.array_equal(np.floor(v + np.float32(0.5)).astype(np.int64), rows)


def test_box_head_on_depth():
    """The box seen head-on: t * (direction in the camera frame)_z of the restatement is the distance of the face's plane."""
    pose = tsdf_ref.look_at((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    intr = (40.0, 40.0, 15.5, 11.5)
    o, d = pv.camera_rays(intr, 24, 32, torch.from_numpy(pose).to(torch.float32))
    local = pv.camera_rays(intr, 24, 32)[1]
    hits = M.cast(M.box(), o.expand_as(d).reshape(-1, 3).numpy(), d.reshape(-1, 3).numpy())
    depth = hits.t[0].reshape(24, 32) * local[..., 2].numpy()
    seen = hits.face[0].reshape(24, 32) >= 0
    assert seen[8:16, 10:22].all() and not seen[0, 0]
    assert np.abs(depth[seen] - 3.0).max() <= 1e-5 * 3.0


# ---------------------------------------------------------------- argument errors, with no GPU
def factory():
    return pv.MeshObjectFactory(mesh=M.box())


def test_cast_rays_argument_errors():
    obj = factory()
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    for bad in ("1", None, True, 1j):
        with pytest.raises(TypeError):
            obj.cast_rays(o, d, t_min=bad)
        with pytest.raises(TypeError):
            obj.cast_rays(o, d, t_max=bad)
    with pytest.raises(ValueError):
        obj.cast_rays(o, d, t_min=math.nan)
    with pytest.raises(ValueError):
        obj.cast_rays(o, d, t_max=math.nan)
    with pytest.raises(ValueError):
        obj.cast_rays(torch.zeros(5, 2), d)
    with pytest.raises(ValueError):
        obj.cast_rays(o, torch.ones(5, 4))
    with pytest.raises(ValueError):
        obj.cast_rays(torch.zeros(4, 3), d)
    for bad in (torch.eye(3), torch.zeros(2, 3, 4), torch.zeros(4)):
        with pytest.raises(ValueError):
            obj.cast_rays(o, d, world_to_object=bad)
    with pytest.raises(ValueError):
        obj.render_depth((1.0, 1.0), 4, 4, torch.eye(4))
    with pytest.raises(ValueError):
        obj.render_depth(INTRINSICS, 4, 4, torch.eye(3))
    with pytest.raises(ValueError):
        obj.render_depth(INTRINSICS, 4, 4, torch.eye(4), max_depth=0.0)
    with pytest.raises(TypeError):
        obj.render_depth(INTRINSICS, 4, 4, torch.eye(4), max_depth="1")


def test_entry_point_argument_errors():
    """The codes of the C entry point that return before any launch."""
    lib = _lib.load()
    desc = _lib.MeshDesc()
    inf = math.inf

    def call(mesh, R, poses, B, t_min=0.0, t_max=inf, rays=1, out=1):
        return lib.pvamd_mesh_ray_cast(ctypes.byref(mesh) if mesh is not None else None, rays, rays, R, poses, B, t_min, t_max, out, out,
                                       None, None, None)

    assert call(desc, -1, None, 1) == _lib.E_SHAPE and call(desc, 4, None, 2) == _lib.E_SHAPE and call(desc, 4, 16, -1) == _lib.E_SHAPE
    assert call(desc, 2 ** 31, None, 1) == _lib.E_SHAPE and call(desc, 2 ** 16, 16, 2 ** 15) == _lib.E_SHAPE
    assert call(None, 4, None, 1) == _lib.H["PVAMD_E_NULL"]
    assert call(desc, 4, None, 1, t_min=math.nan) == _lib.H["PVAMD_E_MODE"] and call(desc, 4, None, 1, t_max=math.nan) == _lib.H["PVAMD_E_MODE"]
    assert call(desc, 0, None, 1) == 0 and call(desc, 4, 16, 0) == 0  # nothing to do: nothing is launched
    assert call(desc, 4, None, 1, rays=None) == _lib.H["PVAMD_E_NULL"] and call(desc, 4, None, 1, out=None) == _lib.H["PVAMD_E_NULL"]
    desc.F = 3
    assert call(desc, 4, None, 1) == _lib.H["PVAMD_E_NULL"]  # faces and no records
    desc.F = -1
    assert call(desc, 4, None, 1) == _lib.E_SHAPE


def test_header_section_and_binding():
    assert _lib.ABI_VERSION == 16 and _lib.load().pvamd_abi_version() == 16
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvamd.h")) as f:
        text = f.read()
    assert "---- Mesh ray casting" in text and re.search(r"u weights corner b, v corner c", text)
    restype, argtypes = _lib.SIGNATURES["pvamd_mesh_ray_cast"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert argtypes[0] is ctypes.POINTER(_lib.MeshDesc) and argtypes[3] is ctypes.c_int64 and argtypes[5] is ctypes.c_int32
    assert argtypes[6] is ctypes.c_float and argtypes[7] is ctypes.c_float
    assert hasattr(_lib.load(), "pvamd_mesh_ray_cast")
    assert pv.MeshRayHits._fields == ("t", "face_ids", "normals", "uv")
