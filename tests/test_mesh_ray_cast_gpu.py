"""-m gpu: ObjectFactory.cast_rays / render_depth and pvamd_mesh_ray_cast, bit for bit against the plain loop over all triangles
(tests/mesh_ray_ref.c), every output included."""
import concurrent.futures
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import mesh_ray_ref as M
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

# 12 triangles: one partial group.  242: one tile, the last group holds 2 records.  288: two tiles, the second nearly all padding.
MESHES = {"box": M.box, "field242": M.field_242, "field288": M.field_288, "drill": M.drill}
H, W = 48, 64


@functools.lru_cache(maxsize=None)
def factory(name):
    mesh = MESHES[name]()
    assert mesh.faces.shape[0] == {"box": 12, "field242": 242, "field288": 288}.get(name, mesh.faces.shape[0])
    return pv.MeshObjectFactory(mesh=mesh)


def centre_extent(name):
    lo, hi = MESHES[name]().aabb()
    return 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))


@functools.lru_cache(maxsize=None)
def image(name):
    """(origins, directions, the restatement's Hits) of a 64 x 48 pinhole image of the mesh with its surroundings; read-only."""
    c, ext = centre_extent(name)
    o, d = M.pinhole(c + ext * np.array([0.9, 0.7, 1.1]), c, H, W, fov=0.6)
    want = M.cast(MESHES[name](), o, d)
    assert 0.15 < (want.face[0] >= 0).mean() < 0.95
    for a in (o, d, *want):
        a.flags.writeable = False
    return o, d, want


def cast(name, o, d, **kwargs):
    return factory(name).cast_rays(torch.from_numpy(np.array(o, np.float32)), torch.from_numpy(np.array(d, np.float32)), **kwargs)


def check(name, o, d, poses=None, t_min=0.0, t_max=math.inf, what=""):
    got = cast(name, o, d, t_min=t_min, t_max=t_max, world_to_object=None if poses is None else torch.from_numpy(np.array(poses)))
    want = M.cast(MESHES[name](), o, d, poses, t_min, t_max)
    M.assert_same(got, want, (name, what))
    return got, want


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("count", [1, 63, 65, H * W])
def test_pinhole_rays(name, count):
    """Diverging rays, whole waves and the tail of one: 1, 63, 65 rays spread over the image, and all of it."""
    o, d, want = image(name)
    pick = np.arange(H * W) if count == H * W else np.linspace(0, H * W - 1, count).astype(np.int64)
    got = cast(name, o[pick], d[pick])
    assert got.t.shape == (count,) and got.face_ids.dtype == torch.int64 and got.normals.shape == (count, 3) and got.uv.shape == (count, 2)
    M.assert_same(got, M.Hits(want.t[:, pick], want.face[:, pick], want.normal[:, pick], want.uv[:, pick]), (name, count))


@pytest.mark.parametrize("name", ["box", "drill"])
def test_rays_from_inside_and_windows(name):
    """Rays that start inside a closed mesh; windows that pass over the first surface so that the second is reported; an empty
    window; directions of length 0.5 and 3."""
    c, ext = centre_extent(name)
    lo, hi = MESHES[name]().aabb()
    rng = np.random.default_rng(11)
    d = rng.standard_normal((130, 3)).astype(np.float32)
    o = np.tile((lo + (hi - lo) * np.array([0.5, 0.5, 0.7])).astype(np.float32), (130, 1))  # in the drill's body
    inside, _ = check(name, o, d, what="inside")
    assert (inside.face_ids >= 0).all()  # a closed mesh is hit in every direction from inside
    o, d, first = image(name)
    o, d = o[::9], d[::9]
    mid = float(np.median(first.t[0][first.face[0] >= 0]))
    got, want = check(name, o, d, t_min=mid, what="t_min")
    moved_on = (want.face[0] >= 0) & (first.face[0][::9] >= 0) & (want.face[0] != first.face[0][::9])
    assert moved_on.sum() > 20  # the first surface was passed over and a later one reported
    check(name, o, d, t_max=mid, what="t_max")
    check(name, o, d, t_min=-10.0 * ext, t_max=mid, what="behind the origin")
    empty, _ = check(name, o, d, t_min=mid, t_max=0.5 * mid, what="t_min > t_max")
    assert (empty.face_ids == -1).all() and torch.isposinf(empty.t).all() and not empty.normals.any() and not empty.uv.any()
    for scale in (0.5, 3.0):
        got, _ = check(name, o, scale * d, what=f"length {scale}")
        hit = first.face[0][::9] >= 0
        assert np.allclose(got.t.numpy()[hit] * scale, first.t[0][::9][hit], rtol=1e-4)


def test_degenerate_rays_on_the_box():
    """Rays in a face's plane (den = 0), at the vertices, along the diagonal two triangles share (ties, U = 0 / V = 0), along
    edges; zero and NaN directions and a NaN origin, next to sound rays in the same wave."""
    box = M.box()
    V = box.vertices.astype(np.float32)
    o, d = [], []
    for v in V:  # at every vertex from three sides and along the body diagonal
        for eye in (v * np.array([1, 1, 4]), v * np.array([4, 1, 1]), v * np.array([1, 4, 1]), v * 3.0, v * np.array([2, 3, 4])):
            o.append(eye)
            d.append(v - eye)
    for s in np.linspace(-1.0, 1.0, 9):  # along both diagonals of the top face and along its edges, from above
        for p in ((s, s, 5.0), (s, -s, 5.0), (s, 1.0, 5.0), (1.0, s, 5.0), (-1.0, s, 5.0)):
            o.append(p)
            d.append((0.0, 0.0, -1.0))
    for y in (-1.0, -0.5, 0.0, 0.25, 1.0):  # in the planes of the top, the bottom and a side face
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
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    got, want = check("box", o, d)
    assert (want.face[0][-7:-1] == -1).all() and want.face[0][-1] >= 0
    assert (want.face[0][:40] >= 0).all()  # every ray at a vertex hits
    check("box", o, d, poses=np.stack([M.rigid(3), np.eye(4, dtype=np.float32)]), what="posed")


@pytest.mark.parametrize("seed", M.IN_PLANE_SEEDS)
def test_rays_in_a_plane_of_a_box_in_general_position(seed):
    """Rays in the plane of a face of a rotated box, up to rounding: den, U, V and T of the face's triangles are rounding noise,
    and the plain loop reports hits with t > 0 for rays that point away from the box with every corner behind the origin, and
    for rays whose line passes more than 3 units beside it.  No geometric cull survives this case; the kernel has none."""
    o, d, away, beside = M.in_plane_rays(seed, 30000)
    mesh = M.rotated_box(seed)
    want = M.cast(mesh, o, d)
    hit = want.face[0] >= 0
    assert (hit & away).sum() >= 5 and (hit & beside).sum() >= 5 and (want.t[0][hit & away] > 0).all()
    obj = pv.MeshObjectFactory(mesh=mesh)
    M.assert_same(obj.cast_rays(torch.from_numpy(o), torch.from_numpy(d)), want, ("in plane", seed))
    pose = M.rigid(seed + 1)[None]
    M.assert_same(obj.cast_rays(torch.from_numpy(o[:4000]), torch.from_numpy(d[:4000]), world_to_object=torch.from_numpy(pose)),
                  M.cast(mesh, o[:4000], d[:4000], pose), ("in plane, posed", seed))


@pytest.mark.parametrize("name", ["box", "field288", "drill"])
def test_eye_far_away(name):
    """An eye 1000 units from the mesh: far rays, whose origins and directions round coarsely against the mesh's size."""
    c, ext = centre_extent(name)
    eye = c + 1000.0 * np.array([0.48, -0.6, 0.64])
    o, d = M.pinhole(eye, c, 24, 32, fov=2.2 * ext / 1000.0)
    got, want = check(name, o, d)
    assert 0.05 < (want.face[0] >= 0).mean()


@pytest.mark.parametrize("name", ["field288", "drill"])
def test_three_poses(name):
    """The identity among three poses gives the bits of the call without poses; shapes (B, ...); float64 rays on the CPU come
    back as float64 on the CPU."""
    o, d, first = image(name)
    o, d = np.array(o[::6]).reshape(16, 32, 3), np.array(d[::6]).reshape(16, 32, 3)
    c, ext = centre_extent(name)
    poses = np.stack([M.rigid(7, 0.1 * ext, about=c), np.eye(4, dtype=np.float32), M.rigid(9, 0.05 * ext, about=c)])
    got, want = check(name, o, d, poses=poses)
    assert got.t.shape == (3, 16, 32) and got.normals.shape == (3, 16, 32, 3) and got.uv.shape == (3, 16, 32, 2)
    plain = cast(name, o, d)
    for a, b in zip(plain, (got.t[1], got.face_ids[1], got.normals[1], got.uv[1])):
        assert np.array_equal(M.bits(a.numpy()), M.bits(b.numpy()))
    assert np.array_equal(M.bits(plain.t.numpy().reshape(-1)), M.bits(first.t[0][::6]))
    assert (want.face[0] >= 0).mean() > 0.1 and (want.face[2] >= 0).mean() > 0.1
    one = factory(name).cast_rays(torch.from_numpy(o[0, 0]).double(), torch.from_numpy(d).double(), world_to_object=torch.from_numpy(poses[0]))
    assert one.t.dtype == torch.float64 and one.t.device.type == "cpu" and one.t.shape == (16, 32) and one.face_ids.dtype == torch.int64
    none = factory(name).cast_rays(torch.zeros(0, 3), torch.zeros(0, 3), world_to_object=torch.from_numpy(poses))
    assert none.t.shape == (3, 0) and none.face_ids.shape == (3, 0) and none.normals.shape == (3, 0, 3) and none.uv.shape == (3, 0, 2)


def raw(name, o, d, poses, normals, uv, F=None, t_min=0.0, t_max=math.inf):
    """pvamd_mesh_ray_cast itself on device tensors; returns (t, face, normal or None, uv or None) as it left them."""
    obj = factory(name)
    desc = obj._mesh_desc()
    if F is not None:
        desc = type(desc).from_buffer_copy(desc)
        desc.F = F
    R, B = o.shape[0], 1 if poses is None else poses.shape[0]
    out = (torch.full((B, R), 7.0, device="cuda"), torch.full((B, R), 7, dtype=torch.int32, device="cuda"),
           torch.full((B, R, 3), 7.0, device="cuda") if normals else None, torch.full((B, R, 2), 7.0, device="cuda") if uv else None)
    run = lambda: _lib.check(_lib.load().pvamd_mesh_ray_cast(ctypes.byref(desc), _lib.ptr(o), _lib.ptr(d), R, _lib.ptr(poses), B, t_min, t_max,
                                                             *map(_lib.ptr, out), _lib.stream_ptr()), "pvamd_mesh_ray_cast")
    run()
    return out, run


def test_optional_outputs_repeat_and_capture():
    """normal_out / uv_out present and absent; two calls give the same bits; the call is captured in a graph (one stream, no
    branches) and its replay gives them again."""
    name = "drill"
    o_np, d_np, want = image(name)
    poses_np = np.stack([M.rigid(8, 0.02), np.eye(4, dtype=np.float32)])
    o, d, poses = (torch.from_numpy(np.array(a)).cuda() for a in (o_np, d_np, poses_np))
    want = M.cast(MESHES[name](), o_np, d_np, poses_np)
    full, _ = raw(name, o, d, poses, True, True)
    for normals, uv in ((False, False), (True, False), (False, True), (True, True)):
        out, _ = raw(name, o, d, poses, normals, uv)
        got = pv.MeshRayHits(out[0], out[1], out[2], out[3])
        M.assert_same(got, M.Hits(want.t, want.face, want.normal if normals else None, want.uv if uv else None), (normals, uv))
    again, _ = raw(name, o, d, poses, True, True)
    for a, b in zip(full, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out, run = raw(name, o, d, poses, True, True)  # warm: the mesh is prepared, the library loaded
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
    for a in out:
        a.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(full, out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_nothing_to_hit():
    """F = 0 misses everywhere and writes every output."""
    o_np, d_np, _ = image("field288")
    o, d = torch.from_numpy(np.array(o_np)).cuda(), torch.from_numpy(np.array(d_np)).cuda()
    (t, face, normal, uv), _ = raw("field288", o, d, None, True, True, F=0)
    assert torch.isposinf(t).all() and (face == -1).all() and not normal.any() and not uv.any()


def test_render_depth_feeds_tsdf_fusion():
    """Six views of the drill at 64 x 48: every image is the restatement's t times the z of the pixel's direction in the camera
    frame, 0 where nothing was hit; TSDFVolume.integrate takes the images as they are and extract_mesh finds a surface."""
    name = "drill"
    c, ext = centre_extent(name)
    poses = torch.from_numpy(tsdf_ref.axis_views(c, 1.6 * ext)).to(torch.float32)
    f = 0.5 * W / math.tan(0.5 * 0.8)
    intrinsics = (f, f, 0.5 * (W - 1), 0.5 * (H - 1))
    depth = factory(name).render_depth(intrinsics, H, W, poses.cuda())
    assert depth.shape == (6, H, W) and depth.dtype == torch.float32 and depth.is_cuda
    origins, directions = pv.camera_rays(intrinsics, H, W, poses.cuda())  # the rays render_depth cast, as the GPU rounded them
    local_z = pv.camera_rays(intrinsics, H, W, torch.eye(4, device="cuda"))[1][..., 2].cpu().numpy()  # the identity turns nothing
    rays = [(origins[k].expand(H, W, 3).cpu().numpy(), directions[k].cpu().numpy()) for k in range(6)]
    with concurrent.futures.ThreadPoolExecutor(6) as pool:  # the restatement's loops run side by side: ctypes releases the GIL
        wants = list(pool.map(lambda od: M.cast(MESHES[name](), od[0], od[1], normals=False, uv=False), rays))
    for k, want in enumerate(wants):
        image_k = np.where(want.face[0].reshape(H, W) >= 0, want.t[0].reshape(H, W) * local_z, np.float32(0))
        assert np.array_equal(M.bits(depth[k].cpu().numpy()), M.bits(image_k.astype(np.float32))), k
        assert 0.02 < (image_k > 0).mean() < 0.9
    near = factory(name).render_depth(intrinsics, H, W, poses[0].cuda(), max_depth=1.6 * ext)
    assert near.shape == (H, W) and (near <= 1.6 * ext).all() and (near > 0).any() and (near == 0).sum() > (depth[0] == 0).sum()
    lo, hi = MESHES[name]().aabb()
    res = float((hi - lo).max()) / 26
    volume = pv.TSDFVolume(res, [(float(lo[k]) - 3 * res, float(lo[k]) + 28 * res) for k in range(3)], truncation=3 * res, device="cuda")
    assert volume.shape == (32, 32, 32)
    volume.integrate(depth, intrinsics, poses.cuda())
    surface = volume.extract_mesh()
    assert surface.vertices.shape[0] > 100 and surface.faces.shape[0] > 100
