"""Mesh-kernel timings for A/B builds: PVAMD_LIB=tools/variants/libpvamd_X.so python tools/ab_mesh.py [bench]"""
import sys, os, time
sys.path.insert(0, os.getcwd())
import torch
import pytorch_volumetric_amd as pv
from pytorch_volumetric_amd import mesh_io
import workloads as H


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def back_to_back(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def median_of(sample, n):
    return sorted(sample() for _ in range(n))[n // 2]


def bench_lines(out, drill, gt, more):
    """The bench's C1 leg (10,000 of the 0.002 m grid points: calls back to back as bench_legs.py times them, and one call between
    HIP events) and its smallest cache build (the drill at 0.01 m: 48,840 voxels through the few-points launch at four waves)."""
    _, g1 = pv.get_coordinates_and_points_in_grid(0.002, drill.bounding_box(0.01))
    c1 = g1[torch.randperm(len(g1), generator=torch.Generator().manual_seed(0))[:10_000]].cuda()
    out.append("bench C1 back to back %.4f ms" % median_of(lambda: back_to_back(lambda: gt(c1), 200), 7 * more))
    out.append("bench C1 one call %.4f ms" % median_of(lambda: timed(lambda: gt(c1), 1), 21 * more))
    build = lambda: pv.CachedSDF("drill_0.01", 0.01, drill.bounding_box(padding=0.1), gt, device="cuda", cache_path=None)
    out.append("build drill_0.01 %.4f ms (min %.4f)" % (median_of(lambda: timed(build, 1), 21 * more), timed(build, 21 * more)))


def main():
    out = []
    if sys.argv[1:] == ["bench"]:  # only the bench-shaped lines, with three times the repeats
        drill = pv.MeshObjectFactory(H.mesh_path("ycb_power_drill.npz"))
        bench_lines(out, drill, pv.MeshSDF(drill), 3)
        print(os.environ.get("PVAMD_LIB", "default"), " | ".join(out))
        return
    sphere = pv.MeshObjectFactory(mesh=mesh_io.uv_sphere_mesh(0.1, 250, 200))
    src = H.uniform_points(1 << 21, [-0.15] * 3, [0.15] * 3, seed=2).cuda()
    W = torch.eye(4).unsqueeze(0).cuda()
    out.append("C5 %.2f ms" % timed(lambda: pv.batch_chamfer_dist(W, src, sphere, scale=1000.0), 4))
    drill = pv.MeshObjectFactory(H.mesh_path("ycb_power_drill.npz"))
    gt = pv.MeshSDF(drill)
    _, grid = pv.get_coordinates_and_points_in_grid(0.002, drill.bounding_box(padding=0.05))
    grid = grid.cuda()
    out.append("drill grid %d pts %.2f ms" % (grid.shape[0], timed(lambda: gt(grid), 4)))
    pts = H.uniform_points(10000, [-0.2] * 3, [0.2] * 3, seed=1).cuda()
    out.append("C1-like 10k random %.3f ms" % timed(lambda: gt(pts), 10))
    big = H.uniform_points(1 << 20, [-0.2] * 3, [0.3] * 3, seed=3).cuda()
    out.append("1M random box %.2f ms" % timed(lambda: gt(big), 3))
    surf, _, _ = pv.sample_mesh_points(drill, num_points=1 << 21, seed=0, dbpath=None, device="cuda")
    surf = (surf + 0.001 * torch.randn_like(surf)).float()
    out.append("2M near-surface chamfer %.2f ms" % timed(lambda: pv.batch_chamfer_dist(W, surf, drill), 3))
    for n in (3_000, 10_000, 30_000, 60_000, 100_000, 200_000):
        q = H.uniform_points(n, [-0.2] * 3, [0.3] * 3, seed=n).cuda()
        out.append("%dk random %.3f ms" % (n // 1000, timed(lambda: gt(q), 6)))
    bench_lines(out, drill, gt, 1)
    print(os.environ.get("PVAMD_LIB", "default"), " | ".join(out))


if __name__ == "__main__":
    main()
