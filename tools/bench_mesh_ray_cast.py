"""ObjectFactory.cast_rays / pvamd_mesh_ray_cast (csrc/mesh_ray.hip) on the drill: 640 x 480 pinhole rays, and 160 x 120 rays under
20 poses, against the only way to cast rays at a mesh before the kernel existed -- MeshSDF(obj).ray_cast, sphere tracing in a torch
loop around the closest-point mesh query, once per pose.  The two do not compute the same thing: the march stops within
hit_tolerance of the surface or after max_steps, cast_rays reports the triangle; the table says how far apart their t are.

Timed with HIP events around the C entry point (and around cast_rays() itself, host work included): median over --calls calls
after a warm-up; the baseline over --baseline-calls calls.  Per case also the ray-triangle tests per second: the kernel tests every
ray against all F triangles.  Prints one JSON line per case and the markdown
table of profiles/mesh_ray_cast.md (--out FILE writes it there too).

The culled contract (cull=True, pvamd_mesh_ray_cast_culled) is timed beside the plain one in the same run, on the same two cases
and on a larger mesh: the drill with every triangle split at its edge midpoints twice, 251,648 triangles.  Per case also the exact
triangle tests per ray of the culled restatement (tests/mesh_ray_cull_ref.c, on the CPU) over a subsample of the rays, and
whether the two kernels gave the same bits.  --out-culled FILE writes profiles/mesh_ray_cast_culled.md.

  python tools/bench_mesh_ray_cast.py [--calls 21] [--baseline-calls 3] [--no-baseline] [--out FILE] [--out-culled FILE]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402
from pytorch_volumetric_amd import mesh_io  # noqa: E402
import workloads  # noqa: E402

# (label, image height, width, poses, times every triangle of the drill is split in four)
CASES = (("640 x 480, no pose", 480, 640, 0, 0), ("160 x 120, 20 poses", 120, 160, 20, 0), ("640 x 480, no pose, drill split twice", 480, 640, 0, 2))
EXPERIMENT_MS = {"640 x 480, no pose": 0.32, "160 x 120, 20 poses": 0.53}  # the dropped culled kernel (profiles/mesh_ray_cast.md)
SUBSAMPLE = 256  # rays the restatement counts exact tests for


def split_in_four(mesh, times):
    """Every triangle split at its edge midpoints, `times` times over: 4^times as many triangles on the same surface."""
    tri = mesh.triangle_soup()
    for _ in range(times):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        tri = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return mesh_io.TriMesh(tri.reshape(-1, 3), np.arange(3 * tri.shape[0]).reshape(-1, 3))


def look_at(eye, target):
    """(4, 4) float64: a camera at `eye` looking along +z at `target`, x right, y down (world up is +z)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, eye
    return pose


def object_poses(B, centre, extent):
    """(B, 4, 4) float32 world_to_object: the object turned about its centre by k / B of a turn about z, and nudged."""
    out = []
    for k in range(B):
        a = 2 * math.pi * k / B
        R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, centre - R @ centre + 0.02 * extent * np.array([math.sin(3 * a), math.cos(2 * a), 0.0])
        out.append(m)
    return torch.from_numpy(np.stack(out)).to(torch.float32)


def timed(fn, calls):
    """Median milliseconds of fn() between HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--out-culled")
    args = ap.parse_args()
    drill = pv.MeshObjectFactory(workloads.mesh_path("ycb_power_drill.npz"))
    lo, hi = drill._mesh.aabb()
    centre, extent = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    objects = {0: drill}
    sdf = pv.MeshSDF(drill)
    lib = _lib.load()
    rows = []
    for label, H, W, B, splits in CASES:
        if splits not in objects:
            objects[splits] = pv.MeshObjectFactory(mesh=split_in_four(drill._mesh, splits))
        obj = objects[splits]
        F = obj.num_faces
        f = 0.5 * W / math.tan(0.5 * 0.7)
        pose = torch.from_numpy(look_at(centre + extent * np.array([0.9, 0.7, 1.1]), centre)).to(torch.float32).cuda()
        origins, directions = pv.camera_rays((f, f, 0.5 * (W - 1), 0.5 * (H - 1)), H, W, pose)
        o = origins.expand_as(directions).reshape(-1, 3).contiguous()
        d = directions.reshape(-1, 3).contiguous()
        poses = object_poses(B, centre, extent).cuda() if B else None
        R, rows_out = o.shape[0], max(B, 1)
        desc = obj._mesh_desc()
        t = torch.empty((rows_out, R), dtype=torch.float32, device="cuda")
        face = torch.empty((rows_out, R), dtype=torch.int32, device="cuda")
        normal = torch.empty((rows_out, R, 3), dtype=torch.float32, device="cuda")
        uv = torch.empty((rows_out, R, 2), dtype=torch.float32, device="cuda")

        def entry():
            _lib.check(lib.pvamd_mesh_ray_cast(ctypes.byref(desc), _lib.ptr(o), _lib.ptr(d), R, _lib.ptr(poses), rows_out, 0.0, math.inf,
                                               _lib.ptr(t), _lib.ptr(face), _lib.ptr(normal), _lib.ptr(uv), _lib.stream_ptr()),
                       "pvamd_mesh_ray_cast")

        def entry_culled():
            _lib.check(lib.pvamd_mesh_ray_cast_culled(ctypes.byref(desc), _lib.ptr(o), _lib.ptr(d), R, _lib.ptr(poses), rows_out, 0.0,
                                                      math.inf, _lib.ptr(t), _lib.ptr(face), _lib.ptr(normal), _lib.ptr(uv), _lib.stream_ptr()),
                       "pvamd_mesh_ray_cast_culled")

        culled_ms = timed(entry_culled, args.calls)
        culled_call_ms = timed(lambda: obj.cast_rays(o, d, world_to_object=poses, cull=True), args.calls)
        culled_out = [a.clone() for a in (t, face, normal, uv)]
        kernel_ms = timed(entry, args.calls)
        call_ms = timed(lambda: obj.cast_rays(o, d, world_to_object=poses), args.calls)
        same_bits = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(culled_out, (t, face, normal, uv)))
        hit = face >= 0
        row = {"case": label, "rays": R, "poses": B, "faces": F, "kernel_ms": round(kernel_ms, 4), "cast_rays_ms": round(call_ms, 4),
               "mrays_per_s": round(rows_out * R / kernel_ms / 1e3, 1), "gtests_per_s": round(rows_out * R * F / kernel_ms / 1e6, 1),
               "hit_fraction": round(float(hit.float().mean()), 4), "culled_kernel_ms": round(culled_ms, 4),
               "culled_cast_rays_ms": round(culled_call_ms, 4), "culled_same_bits": same_bits}
        if args.out_culled:  # the restatement's exact tests per ray, over a subsample of the rays (every pose)
            from tests import mesh_ray_cull_ref
            pick = np.linspace(0, R - 1, SUBSAMPLE).astype(np.int64)
            torch.cuda.synchronize()
            _, tests = mesh_ray_cull_ref.cast(obj._mesh, obj._rec_of_face_dev.cpu().numpy()[:F], obj._tiles_dev.cpu().numpy(),
                                              o.cpu().numpy()[pick], d.cpu().numpy()[pick], None if poses is None else poses.cpu().numpy(),
                                              normals=False, uv=False)
            row["culled_tests_per_ray_mean"], row["culled_tests_per_ray_max"] = round(float(tests.mean()), 1), int(tests.max())
        if not args.no_baseline and splits == 0:
            def march():
                if poses is None:
                    return [sdf.ray_cast(o, d)]
                return [sdf.ray_cast(o @ m[:3, :3].T + m[:3, 3], d @ m[:3, :3].T) for m in poses]

            row["sphere_trace_ms"] = round(timed(march, args.baseline_calls), 3)
            marched = march()
            mt = torch.stack([m.t.reshape(-1) for m in marched])
            mhit = torch.stack([m.status.reshape(-1) == pv.RAY_HIT for m in marched])
            both = hit & mhit
            row["sphere_trace_hit_agreement"] = round(float((hit == mhit).float().mean()), 4)
            row["median_abs_t_difference"] = float((mt[both] - t[both]).abs().median()) if both.any() else None
            row["speedup"] = round(row["sphere_trace_ms"] / kernel_ms, 1)
        rows.append(row)
        print(json.dumps(row))
    lines = ["| case | rays x poses | kernel ms | cast_rays() ms | Mrays/s | G ray-triangle tests/s (F = %d each ray) | MeshSDF.ray_cast ms | "
             "ratio | same hit / miss | median \\|dt\\| |" % drill.num_faces, "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["faces"] != drill.num_faces:
            continue
        lines.append("| %s | %d x %d | %.3f | %.3f | %.0f | %.1f | %s | %s | %s | %s |" % (
            r["case"], r["rays"], max(r["poses"], 1), r["kernel_ms"], r["cast_rays_ms"], r["mrays_per_s"], r["gtests_per_s"],
            r.get("sphere_trace_ms", "-"), r.get("speedup", "-"), r.get("sphere_trace_hit_agreement", "-"),
            "%.2e" % r["median_abs_t_difference"] if r.get("median_abs_t_difference") is not None else "-"))
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# Mesh ray casting (csrc/mesh_ray.hip) on the drill\n\n"
                     "`python tools/bench_mesh_ray_cast.py --out profiles/mesh_ray_cast.md` on one MI355X; medians of %d calls between HIP "
                     "events (the baseline: %d).  kernel: the C entry point alone; cast_rays(): the Python call, its allocations and "
                     "conversions included.  The baseline is MeshSDF(obj).ray_cast on the same rays, once per pose: sphere tracing, which "
                     "stops within hit_tolerance = 1e-3 of the surface or after 128 steps, so its t is not the triangle's.\n\n%s\n"
                     % (args.calls, args.baseline_calls, table))
    lines = ["| case | triangles | rays x poses | plain kernel ms | culled kernel ms | ratio | cast_rays(cull=True) ms | same bits | "
             "exact tests per ray, mean (max) | dropped experiment ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for r in rows:
        lines.append("| %s | %d | %d x %d | %.3f | %.3f | %.1f | %.3f | %s | %s | %s |" % (
            r["case"], r["faces"], r["rays"], max(r["poses"], 1), r["kernel_ms"], r["culled_kernel_ms"], r["kernel_ms"] / r["culled_kernel_ms"],
            r["culled_cast_rays_ms"], "yes" if r["culled_same_bits"] else "NO",
            "%.1f (%d)" % (r["culled_tests_per_ray_mean"], r["culled_tests_per_ray_max"]) if "culled_tests_per_ray_mean" in r else "-",
            EXPERIMENT_MS.get(r["case"], "-")))
        if r["culled_kernel_ms"] >= r["kernel_ms"]:
            notes.append("SLOWER than the plain kernel: %s." % r["case"])
        if r["case"] in EXPERIMENT_MS and r["culled_kernel_ms"] > 2 * EXPERIMENT_MS[r["case"]]:
            notes.append("%s: %.3f ms is more than twice the dropped experiment's %.2f ms." % (r["case"], r["culled_kernel_ms"], EXPERIMENT_MS[r["case"]]))
    culled_table = "\n".join(lines)
    print(culled_table)
    print("\n".join(notes))
    if args.out_culled:
        with open(args.out_culled, "w") as fh:
            fh.write("# Culled mesh ray casting (csrc/mesh_ray.hip, `cull=True`) against the plain kernel\n\n"
                     "`python tools/bench_mesh_ray_cast.py --no-baseline --out-culled profiles/mesh_ray_cast_culled.md` on one MI355X; "
                     "medians of %d calls between HIP events, both kernels in the same run.  kernel: the C entry point alone.  same "
                     "bits: every output of the two entry points compared.  exact tests per ray: triangles whose two spheres the ray "
                     "passes, counted by the restatement (tests/mesh_ray_cull_ref.c) on %d rays spread over the image, every pose.  "
                     "The last case is the drill with every triangle split at its edge midpoints twice.\n\n%s\n\n%s\n"
                     % (args.calls, SUBSAMPLE, culled_table, "\n".join(notes)))


if __name__ == "__main__":
    main()
