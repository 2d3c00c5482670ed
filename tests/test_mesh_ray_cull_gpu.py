"""-m gpu: ObjectFactory.cast_rays / render_depth with cull=True and pvamd_mesh_ray_cast_culled, bit for bit against the
restatement of include/pvamd.h "Mesh ray casting, culled" (tests/mesh_ray_cull_ref.c) on the bounding spheres the library
itself prepared, every output included; and against cull=False on rays in general position."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import _lib
from tests import mesh_ray_cull_ref as C
from tests import mesh_ray_ref as M
from tests import tsdf_ref

pytestmark = pytest.mark.gpu

H, W = C.H, C.W


@functools.lru_cache(maxsize=None)
def factory(name):
    return pv.MeshObjectFactory(mesh=C.MESHES[name]())


def spheres(obj):
    """(rec_of_face, tiles) as pvamd_mesh_prepare left them on the device."""
    F = obj._mesh_desc().F
    torch.cuda.synchronize()
    return obj._rec_of_face_dev.cpu().numpy()[:F], obj._tiles_dev.cpu().numpy()


def test_prepared_spheres_enclose_their_triangles():
    """What the contract's consequences rest on: every corner lies inside the sphere of its record's tile and group."""
    for name in C.MESHES:
        tri = M.soup_of(C.MESHES[name]())[0].astype(np.float64)
        rec_of_face, tiles = spheres(factory(name))
        T = (tri.shape[0] + 255) // 256
        assert tiles.shape[0] >= C.tiles_floats(tri.shape[0])
        for s in (tiles[:4 * T].reshape(T, 4)[rec_of_face // 256], tiles[4 * T:68 * T].reshape(16 * T, 4)[rec_of_face // 16]):
            assert (np.linalg.norm(tri - s[:, None, :3].astype(np.float64), axis=2).max(axis=1) < s[:, 3]).all(), name


def cast(obj, o, d, poses=None, **kwargs):
    return obj.cast_rays(torch.from_numpy(np.array(o, np.float32)), torch.from_numpy(np.array(d, np.float32)),
                         world_to_object=None if poses is None else torch.from_numpy(np.array(poses)), **kwargs)


def check(obj, mesh, o, d, poses=None, t_min=0.0, t_max=math.inf, what="", generic=True):
    """cull=True against the restatement; on a generic set also against cull=False, bit for bit."""
    got = cast(obj, o, d, poses, t_min=t_min, t_max=t_max, cull=True)
    want, tests = C.cast(mesh, *spheres(obj), o, d, poses, t_min, t_max)
    M.assert_same(got, want, what)
    if generic:
        plain = cast(obj, o, d, poses, t_min=t_min, t_max=t_max, cull=False)
        for a, b in zip(got, plain):
            assert a.dtype == b.dtype and np.array_equal(M.bits(a.numpy()), M.bits(b.numpy())), what
    return got, want, tests


@functools.lru_cache(maxsize=None)
def image_want(name):
    """The restatement on the whole 64 x 48 image, once per mesh; read-only."""
    o, d, plain = C.image(name)
    want, tests = C.cast(C.MESHES[name](), *spheres(factory(name)), o, d)
    for a in (*want, tests):
        a.flags.writeable = False
    return want, tests


@pytest.mark.parametrize("name", list(C.MESHES))
@pytest.mark.parametrize("count", [1, 63, 65, H * W])
def test_pinhole_rays(name, count):
    """1, 63, 65 rays spread over the image, and all of it: the tail of a wave, whole waves, waves whose rays pass different
    tiles and groups.  box: one partial group; field242: the last group holds 2 records; field288: a second tile that is nearly
    all padding; drill: 62 tiles."""
    o, d, plain = C.image(name)
    want, tests = image_want(name)
    pick = np.arange(H * W) if count == H * W else np.linspace(0, H * W - 1, count).astype(np.int64)
    got = cast(factory(name), o[pick], d[pick], cull=True)
    assert got.t.shape == (count,) and got.face_ids.dtype == torch.int64 and got.normals.shape == (count, 3) and got.uv.shape == (count, 2)
    M.assert_same(got, M.Hits(want.t[:, pick], want.face[:, pick], want.normal[:, pick], want.uv[:, pick]), (name, count))
    M.assert_same(got, M.Hits(plain.t[:, pick], plain.face[:, pick], plain.normal[:, pick], plain.uv[:, pick]), (name, count, "plain"))
    if name == "drill":
        assert tests.mean() < 0.02 * 15728  # the spheres do cull


@pytest.mark.parametrize("name", ["box", "drill"])
def test_rays_from_inside_and_windows(name):
    for what, o, d, t_min, t_max in C.inside_and_window_cases(name):
        got, want, tests = check(factory(name), C.MESHES[name](), o, d, t_min=t_min, t_max=t_max, what=(name, what))
        if what == "inside":
            assert (got.face_ids >= 0).all()
        if what == "t_min > t_max":
            assert (got.face_ids == -1).all() and torch.isposinf(got.t).all() and not got.normals.any() and not got.uv.any()
        if what == "behind the origin":
            assert (want.face[0] >= 0).any()


def test_degenerate_rays_on_the_box():
    """NaN, infinite and zero rays next to sound ones in one wave; rays in the planes of faces, at vertices, along edges."""
    o, d = C.degenerate_box_rays()
    got, want, tests = check(factory("box"), M.box(), o, d)
    assert (want.face[0][-7:-1] == -1).all() and want.face[0][-1] >= 0 and not tests[0][-7:-1].any()
    assert (want.face[0][:40] >= 0).all()
    check(factory("box"), M.box(), o, d, poses=np.stack([M.rigid(3), np.eye(4, dtype=np.float32)]), what="posed")


@pytest.mark.parametrize("name", ["field288", "drill"])
def test_three_poses(name):
    o, d, _ = C.image(name)
    o, d = np.array(o[::6]).reshape(16, 32, 3), np.array(d[::6]).reshape(16, 32, 3)
    c, ext = C.centre_extent(name)
    poses = np.stack([M.rigid(7, 0.1 * ext, about=c), np.eye(4, dtype=np.float32), M.rigid(9, 0.05 * ext, about=c)])
    got, want, _ = check(factory(name), C.MESHES[name](), o, d, poses=poses, what=name)
    assert got.t.shape == (3, 16, 32) and got.normals.shape == (3, 16, 32, 3) and got.uv.shape == (3, 16, 32, 2)
    assert (want.face[0] >= 0).mean() > 0.1 and (want.face[2] >= 0).mean() > 0.1
    unposed = cast(factory(name), o, d, cull=True)
    for a, b in zip(unposed, (got.t[1], got.face_ids[1], got.normals[1], got.uv[1])):
        assert np.array_equal(M.bits(a.numpy()), M.bits(b.numpy()))


def test_rays_in_a_plane_of_a_box_in_general_position():
    """The rays on which the two contracts differ: the kernel follows the culled restatement, plain and posed, and drops most of
    what the plain call reports."""
    seed = M.IN_PLANE_SEEDS[0]
    o, d, away, beside = M.in_plane_rays(seed, 30000)
    mesh = M.rotated_box(seed)
    obj = pv.MeshObjectFactory(mesh=mesh)
    got, want, _ = check(obj, mesh, o, d, what="in plane", generic=False)
    plain = cast(obj, o, d)
    assert (plain.face_ids >= 0).sum() >= 10 and (got.face_ids >= 0).sum() < (plain.face_ids >= 0).sum()
    kept = (got.face_ids >= 0).numpy()
    for a, b in zip(got, plain):  # what it keeps is the plain call's
        assert np.array_equal(M.bits(a.numpy()[kept]), M.bits(b.numpy()[kept]))
    check(obj, mesh, o[:4000], d[:4000], poses=M.rigid(seed + 1)[None], what="in plane, posed", generic=False)


def test_cull_argument():
    """cull=False is the call without the argument; anything but a bool is a TypeError."""
    o, d, plain = C.image("field288")
    obj = factory("field288")
    for a, b in zip(cast(obj, o, d), cast(obj, o, d, cull=False)):
        assert np.array_equal(M.bits(a.numpy()), M.bits(b.numpy()))
    M.assert_same(cast(obj, o, d, cull=False), plain)
    for bad in (1, None, "yes", np.True_):
        with pytest.raises(TypeError):
            cast(obj, o, d, cull=bad)
        with pytest.raises(TypeError):
            obj.render_depth((60.0, 60.0, 31.5, 23.5), H, W, torch.eye(4), cull=bad)


def raw(name, o, d, poses, normals, uv):
    """pvamd_mesh_ray_cast_culled itself on device tensors; returns (t, face, normal or None, uv or None) and the call."""
    desc = factory(name)._mesh_desc()
    R, B = o.shape[0], 1 if poses is None else poses.shape[0]
    out = (torch.full((B, R), 7.0, device="cuda"), torch.full((B, R), 7, dtype=torch.int32, device="cuda"),
           torch.full((B, R, 3), 7.0, device="cuda") if normals else None, torch.full((B, R, 2), 7.0, device="cuda") if uv else None)
    run = lambda: _lib.check(_lib.load().pvamd_mesh_ray_cast_culled(ctypes.byref(desc), _lib.ptr(o), _lib.ptr(d), R, _lib.ptr(poses), B, 0.0,
                                                                    math.inf, *map(_lib.ptr, out), _lib.stream_ptr()),
                             "pvamd_mesh_ray_cast_culled")
    run()
    return out, run


def test_optional_outputs_repeat_and_capture():
    """normal_out / uv_out present and absent at the C entry; two calls give the same bits; the call is captured in a graph (one
    stream, no branches) and its replay gives them again."""
    name = "drill"
    o_np, d_np, _ = C.image(name)
    poses_np = np.stack([M.rigid(8, 0.02), np.eye(4, dtype=np.float32)])
    o, d, poses = (torch.from_numpy(np.array(a)).cuda() for a in (o_np, d_np, poses_np))
    want, _ = C.cast(C.MESHES[name](), *spheres(factory(name)), o_np, d_np, poses_np)
    full, _ = raw(name, o, d, poses, True, True)
    for normals, uv in ((False, False), (True, False), (False, True), (True, True)):
        out, _ = raw(name, o, d, poses, normals, uv)
        M.assert_same(pv.MeshRayHits(*out), M.Hits(want.t, want.face, want.normal if normals else None, want.uv if uv else None), (normals, uv))
    again, _ = raw(name, o, d, poses, True, True)
    for a, b in zip(full, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out, run = raw(name, o, d, poses, True, True)  # warm
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


def test_render_depth_of_a_fused_ball():
    """TSDFVolume of a small ball -> extract_mesh -> MeshObjectFactory -> render_depth: one 64 x 48 view, culled and not, the
    same bits."""
    radius, res, intrinsics = 0.3, 0.04, (150.0, 150.0, 79.5, 59.5)
    poses = tsdf_ref.axis_views((0.0, 0.0, 0.0), 1.0)
    depth = tsdf_ref.ball_depth(poses, intrinsics, 120, 160, (0.0, 0.0, 0.0), radius)
    volume = pv.TSDFVolume(res, [(-0.5, 0.5)] * 3, truncation=3 * res, device="cuda")
    volume.integrate(torch.from_numpy(depth), intrinsics, torch.from_numpy(poses))
    mesh = volume.extract_mesh().to_trimesh()
    assert mesh.faces.shape[0] > 256  # more than one tile
    obj = pv.MeshObjectFactory(mesh=mesh)
    f = 0.5 * W / math.tan(0.5 * 0.9)
    view = (f, f, 0.5 * (W - 1), 0.5 * (H - 1))
    pose = torch.from_numpy(tsdf_ref.look_at((0.9, 0.6, 0.7), (0.0, 0.0, 0.0))).to(torch.float32).cuda()
    plain = obj.render_depth(view, H, W, pose)
    culled = obj.render_depth(view, H, W, pose, cull=True)
    assert culled.shape == (H, W) and culled.dtype == torch.float32 and culled.is_cuda
    assert torch.equal(plain.view(torch.int32), culled.view(torch.int32))
    assert 0.05 < float((culled > 0).float().mean()) < 0.9
    assert float((culled[culled > 0] - (math.sqrt(0.9 ** 2 + 0.6 ** 2 + 0.7 ** 2) - radius)).min()) > -2 * res  # a ball at the right place
