"""Nearest vs trilinear (interpolation="trilinear") on the C2 cache and the C4 robot: HIP-event timings after a warm-up, median
of --regions regions, the two modes alternated in one process on the same inputs.  Prints one JSON line per case and a table.

  python tools/bench_interp.py [--regions 21] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import workloads as W  # noqa: E402


def region_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(fns, regions, iters):
    for fn in fns.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            times[k].append(region_ms(fn, iters))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []

    near, tri = W.build_c2_cache(), W.build_c2_cache()
    tri.interpolation = "trilinear"
    P = 1 << 20
    for name, pts in (("C2 headline mix", W.c2_points(near, P, seed=0)), ("C2 all in range", W.c2_points(near, P, seed=0, margin=-0.02))):
        fwd = alternate({"nearest": lambda: near(pts), "trilinear": lambda: tri(pts)}, args.regions, args.iters)
        pg = pts.clone().requires_grad_()

        def fb(c):
            def run():
                pg.grad = None
                v, g = c(pg)
                (v.sum() + g.sum()).backward()
            return run
        fb_t = alternate({"nearest": fb(near), "trilinear": fb(tri)}, args.regions, max(1, args.iters // 4))
        rows.append({"case": name, "points": P, "fwd_ms": fwd, "fwd_bwd_ms": fb_t,
                     "fwd_frac_8TBs": {k: 28 * P / (v * 1e-3) / 8e12 for k, v in fwd.items()}})

    robots = {"nearest": W.build_c4()}
    import tempfile
    import pytorch_volumetric_amd as pv
    with tempfile.TemporaryDirectory() as tmp:
        chain = W.synthetic_arm(tmp)
        robots["trilinear"] = pv.RobotSDF(chain, path_prefix=tmp, link_sdf_cls=pv.cache_link_sdf_factory(
            0.02, 0.1, device="cuda", cache_path=None, interpolation="trilinear"))
    A, P = 200, 262144
    q = W.c4_joint_configs(A, seed=0).cuda()
    pts = W.c4_points(P, seed=1)
    for r in robots.values():
        r.set_joint_configuration(q)
    fwd = alternate({k: (lambda r=r: r(pts)) for k, r in robots.items()}, args.regions, max(1, args.iters // 4))

    def fbq(r):
        def run():
            qq = q.clone().requires_grad_()
            r.set_joint_configuration(qq)
            v, g = r(pts)
            v.sum().backward()
        return run
    fb_t = alternate({k: fbq(r) for k, r in robots.items()}, max(5, args.regions // 2), 1)
    rows.append({"case": "C4 robot", "configs": A, "points": P, "fwd_ms": fwd, "fwd_bwd_q_ms": fb_t,
                 "fwd_frac_8TBs": {k: 28 * A * P / (v * 1e-3) / 8e12 for k, v in fwd.items()}})

    for row in rows:
        print(json.dumps(row))
    print(f"{'case':18s} {'mode':10s} {'fwd ms':>9s} {'x nearest':>9s} {'fwd+bwd ms':>11s}")
    for row in rows:
        fbk = "fwd_bwd_ms" if "fwd_bwd_ms" in row else "fwd_bwd_q_ms"
        for k in ("nearest", "trilinear"):
            print(f"{row['case']:18s} {k:10s} {row['fwd_ms'][k]:9.4f} {row['fwd_ms'][k] / row['fwd_ms']['nearest']:9.2f} "
                  f"{row[fbk][k]:11.3f}")


if __name__ == "__main__":
    main()
