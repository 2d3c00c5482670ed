"""Eager wall time per call of the paths whose scratch is sized by the library's mesh and sort size functions: the C1 mesh query,
one cache build, one spatial sort, and bench.py's C1 leg (bench_legs.leg_c1, called as bench.py calls it).  argv[1]: the tree
whose package to import (this repository, or a checkout of another commit built the same way), argv[2]: output JSON."""
import json
import os
import statistics
import sys
import time

tree = os.path.abspath(sys.argv[1])
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench_legs  # noqa: E402
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402
from pytorch_volumetric_amd import _lib  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(pv.__file__))) == tree, pv.__file__
assert os.path.dirname(os.path.abspath(bench_legs.__file__)) == tree, bench_legs.__file__


def per_call_us(fn, calls, regions):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return statistics.median(out)


torch.cuda.set_device(0)
drill = W.build_drill()
sdf = pv.MeshSDF(drill)
_, grid_pts = pv.get_coordinates_and_points_in_grid(0.002, drill.bounding_box(0.01))
pts = grid_pts[torch.randperm(len(grid_pts), generator=torch.Generator().manual_seed(0))[:10_000]].cuda()
cloud = (torch.rand(100_000, 3, generator=torch.Generator().manual_seed(1)) - 0.5).cuda()
name, _, res, pad, _ = bench_legs.CACHE_BUILDS[0]
ranges = drill.bounding_box(padding=pad)
res_us = {}
with torch.no_grad():
    res_us["MeshSDF(drill)(10,000 points)"] = per_call_us(lambda: sdf(pts), 200, 9)
    res_us[f"CachedSDF build {name}"] = per_call_us(lambda: pv.CachedSDF("drill", res, ranges, sdf, device="cuda", cache_path=None), 20, 9)
    res_us["morton_order 100,000 points"] = per_call_us(lambda: _lib.morton_order(cloud), 200, 9)
    res_us["bench legs.c1 ms_per_call"] = bench_legs.leg_c1(torch, np, W, pv, lambda: None, 1)["ms_per_call"] * 1e3
json.dump(res_us, open(sys.argv[2], "w"), indent=1)
print(json.dumps(res_us))
