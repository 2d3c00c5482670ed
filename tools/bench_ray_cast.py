"""ray_cast (csrc/ray_cast.hip) against what a caller writes without it -- the step loop in torch around __call__, with the same
arguments: every step forms the points of all rays, queries them, and torch.where keeps the finished rays; it stops (one device ->
host read per step) when no ray is marching.  HIP-event timings after a warm-up, median of --regions regions, the two variants
alternated in one process on the same rays.  Cases: 640 x 480 pinhole rays at the drill cache (0.01 m), nearest and trilinear; 160 x
120 rays at the C4 robot (W.build_c4, 8 links of 100 KB) under A = 20 configurations, where the loop runs one configuration at a
time as the one-configuration composition of its rows.  Prints one JSON line per case and the markdown table of
profiles/ray_cast.md (--out FILE writes the table there too).

  python tools/bench_ray_cast.py [--regions 9] [--iters 3] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import workloads as W  # noqa: E402
import pytorch_volumetric_amd as pv  # noqa: E402

T_MAX, TOL, MAX_STEPS = 3.0, 1e-3, 128


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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            times[k].append(region_ms(fn, iters))
    return {k: statistics.median(v) for k, v in times.items()}


def pinhole(width, height, eye, target, fov_x_deg):
    """(height, width, 3) unit directions of a pinhole camera at `eye` looking at `target`, z up; plain torch."""
    eye, target = torch.tensor(eye, dtype=torch.float32), torch.tensor(target, dtype=torch.float32)
    f = torch.nn.functional.normalize(target - eye, dim=0)
    r = torch.nn.functional.normalize(torch.linalg.cross(f, torch.tensor([0.0, 0.0, 1.0])), dim=0)
    u = torch.linalg.cross(r, f)
    half = math.tan(math.radians(fov_x_deg) / 2)
    xs = torch.linspace(-half, half, width)
    ys = torch.linspace(half * height / width, -half * height / width, height)
    d = f + xs[None, :, None] * r + ys[:, None, None] * u
    return eye.cuda(), torch.nn.functional.normalize(d, dim=-1).cuda().contiguous()


def step_loop(sdf, o, d):
    """The loop over __call__ for (R, 3) rays: (t, status, steps)."""
    R = o.shape[0]
    t = torch.zeros(R, device=o.device)
    steps = torch.zeros(R, dtype=torch.int32, device=o.device)
    status = torch.full((R,), pv.RAY_MAX_STEPS, dtype=torch.uint8, device=o.device)
    active = torch.ones(R, dtype=torch.bool, device=o.device)
    for _ in range(MAX_STEPS):
        if not bool(active.any()):
            break
        v, _ = sdf(o + t.unsqueeze(-1) * d)
        v = v.reshape(R)
        steps = steps + active.int()
        nan = v != v
        hit = ~nan & (v <= TOL)
        tn = t + v
        miss = ~nan & ~hit & ~(tn <= T_MAX)
        for code, stop in ((pv.RAY_INVALID, nan), (pv.RAY_HIT, hit), (pv.RAY_MISS, miss)):
            status = torch.where(active & stop, torch.tensor(code, dtype=torch.uint8, device=o.device), status)
        active = active & ~nan & ~hit & ~miss
        t = torch.where(active, tn, t)
    return t, status, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file (profiles/ray_cast.md holds it with its notes)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []

    def case(name, sdf, singles, eye, dirs):
        o = eye.expand_as(dirs).reshape(-1, 3).contiguous()
        d = dirs.reshape(-1, 3)
        res = sdf.ray_cast(eye, dirs, t_max=T_MAX, hit_tolerance=TOL, max_steps=MAX_STEPS)
        loop = [step_loop(one, o, d) for one in singles]
        same = all(torch.equal(res.status.reshape(len(singles), -1)[a], loop[a][1]) and
                   torch.equal(res.steps.reshape(len(singles), -1)[a], loop[a][2]) for a in range(len(singles)))
        t = alternate({"loop": lambda: [step_loop(one, o, d) for one in singles],
                       "fused": lambda: sdf.ray_cast(eye, dirs, t_max=T_MAX, hit_tolerance=TOL, max_steps=MAX_STEPS)},
                      args.regions, args.iters)
        rows.append({"case": name, "configs": len(singles), "rays": d.shape[0], "loop_ms": t["loop"], "fused_ms": t["fused"],
                     "fused_over_loop": t["fused"] / t["loop"], "mean_steps": float(res.steps.float().mean()),
                     "max_steps_taken": int(res.steps.max()), "hit_fraction": float((res.status == pv.RAY_HIT).float().mean()),
                     "loop_agrees": same})

    for mode in ("nearest", "trilinear"):
        c = W.build_c2_cache()
        c.interpolation = mode
        centre = [(r[0] + r[1]) / 2 for r in c.ranges]
        eye, dirs = pinhole(640, 480, [centre[0] + 0.55, centre[1] + 0.2, centre[2] + 0.12], centre, 50.0)
        case(f"drill cache 0.01 m, {mode}", c, [c], eye, dirs)

    robot = W.build_c4()
    A = 20
    robot.set_joint_configuration(W.c4_joint_configs(A, seed=0).cuda())
    comp = robot.sdf
    stack = comp._tf_matrix.detach().reshape(len(comp.sdfs), A, 4, 4)
    singles = []
    for a in range(A):
        one = pv.ComposedSDF(comp.sdfs, None)
        one.set_transforms(stack[:, a].contiguous(), known_rigid=True)
        singles.append(one)
    eye, dirs = pinhole(160, 120, [1.2, 0.5, 0.8], [0.0, 0.0, 0.6], 70.0)
    case("C4 robot, nearest", robot, singles, eye, dirs)

    for row in rows:
        print(json.dumps(row))
    lines = ["| case | configurations x rays | step loop over `__call__` ms | fused `ray_cast` ms | fused / loop | mean steps per ray | "
             "most steps | rays that hit |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['configs']} x {r['rays']:,} | {r['loop_ms']:.3f} | {r['fused_ms']:.4f} | "
                     f"{r['fused_over_loop']:.4f} | {r['mean_steps']:.1f} | {r['max_steps_taken']} | {100 * r['hit_fraction']:.1f} % |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
