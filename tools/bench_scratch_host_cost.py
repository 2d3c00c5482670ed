"""Eager wall time per call of the four fused reductions at their bench shapes.  argv[1]: the tree whose package to import
(this repository, or a checkout of another commit built the same way), argv[2]: output JSON."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
sys.path.insert(0, tree)
import torch  # noqa: E402
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(pv.__file__))) == tree, pv.__file__


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
r = W.build_c4()
pairs = r.self_collision_pairs()
res = {}
with torch.no_grad():
    for A in (1, 200):
        q = W.c4_joint_configs(A, seed=0).cuda()
        r.set_joint_configuration(q[0] if A == 1 else q)
        for P in (16384, 262144):
            pts = W.c4_points(P, seed=1)
            calls = 200 if A == 1 else 20
            res[f"min_over_points A={A} P={P}"] = per_call_us(lambda: r.sdf.min_over_points(pts), calls, 9)
            res[f"hinge_over_points A={A} P={P}"] = per_call_us(lambda: r.sdf.hinge_over_points(pts, 0.2), calls, 9)
        for npts in (256, 1024):
            r.set_self_collision_points(num_points=npts, seed=0)
            sets = r._sc_points
            calls = 200 if A == 1 else 50
            res[f"leaf_pair_distance A={A} pts={npts}"] = per_call_us(lambda: r.sdf.leaf_pair_distance(sets, pairs), calls, 9)
            res[f"leaf_pair_hinge A={A} pts={npts}"] = per_call_us(lambda: r.sdf.leaf_pair_hinge(sets, pairs, 0.2, 2), calls, 9)
json.dump(res, open(sys.argv[2], "w"), indent=1)
print(json.dumps(res))
